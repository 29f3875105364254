"""Child process of tests/test_gpu_densecl.py: four DenseCL steps through graph.StepGraph under the SSV_STEP_GRAPH value of its environment (the module reads it
at import), with the eager kernel selection (graph_floors=False: replayed steps are then the eager steps bit for bit).  Usage:
    python densecl_steps_child.py <config.yaml> <out.pt>          (run from the directory the outputs/ tree may be written to)
Writes {"losses", "flags" (the dense loss's flag after every step), "lse" (the dense loss's lse after every step), "queue_ptr" and "dense_ptr" (both queue
pointers after every step), "graph" (StepGraph.describe())}."""
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
    t = cli.trainer_class("densecl")(args={"config": config, "arch": "resnet18", "algo": "densecl", "task": "train", "output": "steps", "load": None})
    b = t.config["data"]["batch_size"]
    sg = StepGraph(t, graph_floors=False)
    res = {"losses": [], "flags": [], "lse": [], "queue_ptr": [], "dense_ptr": []}
    for i in range(4):
        batch = {"aug_1": seeded_randn(300 + 2 * i, b, 3, 32, 32).to(dev), "aug_2": seeded_randn(301 + 2 * i, b, 3, 32, 32).to(dev), "label": torch.zeros(b)}
        res["losses"].append(sg(batch)["loss"])
        torch.cuda.synchronize()
        res["flags"].append(int(t.dense_loss_fn.last_flag.item()))
        res["lse"].append(t.dense_loss_fn.last_lse.detach().cpu().clone())
        res["queue_ptr"].append(t.memory_bank.ptr)
        res["dense_ptr"].append(t.dense_bank.ptr)
    res["graph"] = sg.describe()
    sg.close()
    torch.save(res, out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
