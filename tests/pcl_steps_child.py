"""Child process of tests/test_gpu_pcl.py: an E-step, then four PCL steps (InfoNCE + ProtoNCE) through graph.StepGraph under the SSV_STEP_GRAPH value of its
environment (the module reads it at import), with the eager kernel selection (graph_floors=False: replayed steps are then the eager steps bit for bit).  Usage:
    python pcl_steps_child.py <config.yaml> <out.pt>          (run from the directory the outputs/ tree may be written to)
Writes {"losses", "flags" (the ProtoNCE flag after every step), "lse" (the last ProtoNCE call's lse after every step), "queue_ptr", "graph" (StepGraph.describe())}."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(config, out):
    import torch
    from conftest import seeded_randn
    from ssv_amd import main as cli
    from ssv_amd.graph import StepGraph
    dev = torch.device("cuda", 0)
    torch.manual_seed(420)
    t = cli.trainer_class("pcl")(args={"config": config, "arch": "resnet18", "algo": "pcl", "task": "train", "output": "steps", "load": None})
    b, n = t.config["data"]["batch_size"], t.train_loader.shape[0]
    t.e_step()
    sg = StepGraph(t, graph_floors=False)
    res = {"losses": [], "flags": [], "lse": [], "queue_ptr": []}
    for i in range(4):
        index = ((torch.arange(b) * 3 + 5 * i) % n).to(dev)
        batch = {"aug_1": seeded_randn(300 + 2 * i, b, 3, 32, 32).to(dev), "aug_2": seeded_randn(301 + 2 * i, b, 3, 32, 32).to(dev), "index": index, "label": torch.zeros(b)}
        res["losses"].append(sg(batch)["loss"])
        torch.cuda.synchronize()
        res["flags"].append(int(t.proto_loss_fn.last_flag.item()))
        res["lse"].append(t.proto_loss_fn.last_lse.detach().cpu().clone())
        res["queue_ptr"].append(t.memory_bank.ptr)
    res["graph"] = sg.describe()
    sg.close()
    torch.save(res, out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
