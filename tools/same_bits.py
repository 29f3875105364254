#!/usr/bin/env python3
"""Do two builds of libssv_hip.so give the same bytes?  For each library a fresh child process (the library selected through SSV_HIP_LIB, the child under its own
time limit) runs ssv_proto_nce, ssv_queue_nce and ssv_nn_lookup through the guarded C-ABI calls of the forms tests (tests/test_gpu_proto_nce_forms.py,
tests/test_gpu_dense_nce_forms.py, tests/test_gpu_nn_lookup_forms.py: guards, NaN tails and a prefilled workspace, all verified) in both arithmetics over the
committed case tables - pcl_oracle.cases() + FORM_CASES, densecl_oracle.cases() + FORM_CASES, nnclr_oracle.LOOKUP_CASES + FORM_LOOKUP_CASES - and dumps loss, lse,
dq and flag (the lookup: idx, sim, nn).  The dumps are compared byte for byte; there is no tolerance.
    python tools/same_bits.py OLD_LIB NEW_LIB [-o report.json]
Exit status 1 if a case differs; the first child that does not exit 0 ends the run with status 2."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CHILD_SECONDS = 480
ARITHS = ("bf16x3", "f32")


def dump(path):
    """the child: every case in both arithmetics on the library SSV_HIP_LIB names -> one .npz of raw arrays, keyed family/arithmetic/case/output"""
    import numpy as np
    import torch
    import densecl_oracle as do
    import nnclr_oracle as no
    import pcl_oracle as po
    import test_gpu_dense_nce_forms as qn
    import test_gpu_nn_lookup_forms as nn
    import test_gpu_proto_nce_forms as pn
    from ssv_amd import _lib
    assert torch.cuda.is_available(), "same_bits.py runs on the GPU; none is visible"
    lib = _lib.load()
    out = {}
    for arith in ARITHS:
        for fam, mod, oracle in (("proto_nce", pn, po), ("queue_nce", qn, do)):
            for case in oracle.cases() + oracle.FORM_CASES:
                what = f"{fam}/{arith}/{oracle.case_id(case)}"
                got = mod._call(lib, oracle.make_case(case), arith, mod.FILLS[0], what)
                for k in ("loss", "lse", "dq"):
                    out[f"{what}/{k}"] = got[k].numpy()
                out[f"{what}/flag"] = np.int32(got["flag"])
        for name, c in {**no.LOOKUP_CASES, **no.FORM_LOOKUP_CASES}.items():
            what = f"nn_lookup/{arith}/{name}"
            q, b = no.lookup_inputs(name)
            rows, idx, sim = nn._lookup(lib, q, b, c.n, arith, 10.0, nn.FILLS[0], what)
            out.update({f"{what}/nn": rows, f"{what}/idx": idx, f"{what}/sim": sim})
    np.savez(path, **out)
    print("SHA " + _lib.source_sha16())


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old", nargs="?")
    ap.add_argument("new", nargs="?")
    ap.add_argument("-o", "--out")
    ap.add_argument("--dump", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.dump:
        dump(a.dump)
        return 0
    import numpy as np
    assert a.old and a.new, "two libraries to compare"
    shas, dumps = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, lib in (("parent", a.old), ("new", a.new)):
            path = os.path.join(tmp, tag + ".npz")
            try:
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", path], env=dict(os.environ, SSV_HIP_LIB=os.path.abspath(lib)),
                                     capture_output=True, text=True, timeout=CHILD_SECONDS)
            except subprocess.TimeoutExpired:
                sys.stderr.write(f"the child on {lib} ran into its time limit of {CHILD_SECONDS} s: nothing more is run\n")
                return 2
            if res.returncode != 0:
                sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:] + f"\nthe child on {lib} failed (rc {res.returncode}): nothing more is run\n")
                return 2
            shas[tag] = [ln for ln in res.stdout.splitlines() if ln.startswith("SHA ")][-1][4:]
            with np.load(path) as z:
                dumps[tag] = {k: z[k] for k in z.files}
    old, new = dumps["parent"], dumps["new"]
    assert set(old) == set(new), "the two libraries ran different cases"
    cases = {}
    for key in sorted(old):
        case, name = key.rsplit("/", 1)
        same = old[key].dtype == new[key].dtype and old[key].shape == new[key].shape and old[key].tobytes() == new[key].tobytes()
        e = cases.setdefault(case, {"arrays": 0, "bytes": 0, "identical": True})
        e["arrays"] += 1
        e["bytes"] += old[key].nbytes
        if not same:
            e["identical"] = False
            e.setdefault("differs", []).append(name)
    ok = all(e["identical"] for e in cases.values())
    doc = {"what": "outputs of two builds of the library on the same seeded inputs, each library in a fresh process (selected through SSV_HIP_LIB), through the guarded "
                   "C-ABI calls of the forms tests in both arithmetics; the dumped arrays (loss, lse, dq, flag; the lookup: idx, sim, nn) are compared byte for byte",
           "ssv_source_sha16": shas, "cases_compared": len(cases), "all_identical": ok, "cases": cases}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    for case, e in cases.items():
        if not e["identical"]:
            print(f"DIFFERENT {case}: {e['differs']}")
    print(f"{len(cases)} cases, {sum(e['identical'] for e in cases.values())} identical; parent {shas['parent']}, new {shas['new']}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
