#!/usr/bin/env python3
"""Do two builds of libssv_hip.so give the same bytes?  For each library a fresh child process (the library selected through SSV_HIP_LIB, the child under its own
time limit) runs ssv_proto_nce, ssv_queue_nce and ssv_nn_lookup through the guarded C-ABI calls of the forms tests (tests/test_gpu_proto_nce_forms.py,
tests/test_gpu_dense_nce_forms.py, tests/test_gpu_nn_lookup_forms.py: guards, NaN tails and a prefilled workspace, all verified) in both arithmetics over the
committed case tables - pcl_oracle.cases() + FORM_CASES, densecl_oracle.cases() + FORM_CASES, nnclr_oracle.LOOKUP_CASES + FORM_LOOKUP_CASES - and dumps loss, lse,
dq and flag (the lookup: idx, sim, nn).  The Winograd stages: every `filt`, `in`, `dy` and `out` case of tests/test_gpu_wino_forms.CASES through the calling half of
that file's runners (the same guarded buffers, guards and identities verified), every array they return dumped - U, dw, V, V2, dM, Vd, y, both partial pairs - with
the library's host answers.  Attention: every case of kind afwd, abwd and acomp of tests/test_gpu_vit_kernels.CASES through that file's guarded callers (forward in
both arithmetics, the backward forms; guards, NaN padding columns and the stated identities verified in both children), every array they return dumped - o_*,
lse_*, delta, dq, dk, dv and the composed gradients - as attention/<case id>/<name>.  BatchNorm and pooling: every case of tests/test_gpu_bn_pool_kernels.CASES
through that file's guarded runners (guards, untouched inputs and the stated bitwise identities verified in both children), every tensor they return dumped as
bn_pool/<case id>/<name>; an array above 16 MB is recorded as the sha256 of its bytes with its shape and dtype, which compares just as exactly.  The dumps are
compared byte for byte; there is no tolerance.
    python tools/same_bits.py OLD_LIB NEW_LIB [-o report.json] [--old-root DIR]
--old-root DIR: the old library's child imports the package from DIR (a checkout of the parent commit), the new library's from this tree, and both also run the
chain table below through ops.wino_conv2d_fwd / _dgrad / _wgrad under ops.large_batch_dispatch() in both arithmetics: a rewrite of the Python drivers is compared
like a rewrite of the kernels.  Exit status 1 if a case differs; the first child that does not exit 0 ends the run with status 2."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the package comes from SSV_SAME_BITS_ROOT (the old library's child under --old-root) or from this tree; the case tables and guarded runners always from this tree
sys.path[:0] = [os.environ.get("SSV_SAME_BITS_ROOT") or ROOT, os.path.join(ROOT, "tests")]
CHILD_SECONDS = 480
BIG_BYTES = 16 << 20                                 # a larger array is dumped as its sha256
ARITHS = ("bf16x3", "f32")
# the chain table: maps (6x6 has ratio 1.0 and stays on F(2x2) with F(4x4) on; 7x7 and 8x8 take F(4x4)), (N, C, K), and the switch that is off (None: the defaults)
CHAIN_MAPS, CHAIN_NCK = ((6, 6), (7, 7), (8, 8)), ((3, 32, 64), (2, 64, 32), (2, 128, 128))
CHAIN_OFF = (None, "WINOGRAD44", "WINOGRAD44_WGRAD", "WINOGRAD44_DY_BOTH")


def chains(ops, dev, arith, out):
    """forward plain / with statistics / with the fused input / keeping V, data gradient plain / affine gate / mask gate, weight gradient overwriting and
    accumulating, and (defaults only, where the forward kept F(4x4)'s V) one LazyGrad weight gradient followed by its data gradient"""
    import torch
    import wino_oracle as wo

    def put(what, name, t):
        out[f"wino_chain/{arith}/{what}/{name}"] = t.detach().cpu().numpy()

    for off in CHAIN_OFF:
        prev = getattr(ops, off) if off else None
        if off:
            setattr(ops, off, False)
        try:
            for (h, w_) in CHAIN_MAPS:
                for (n, c, k) in CHAIN_NCK:
                    what = f"{off or 'defaults'}-{n}x{h}x{w_}-C{c}-K{k}"
                    g = torch.Generator().manual_seed(1000 * h + 10 * c + k)
                    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)          # noqa: E731
                    x, dy, gx = rn(n, h, w_, c), rn(n, h, w_, k), rn(n, h, w_, c)
                    w = rn(k, c, 3, 3, scale=(2.0 / (9 * c)) ** 0.5).contiguous(memory_format=torch.channels_last)
                    sc, sh = (torch.rand(c, generator=g) + 0.5).to(dev), rn(c, scale=0.3)
                    mean, invstd = rn(c, scale=0.2), (torch.rand(c, generator=g) + 0.5).to(dev)
                    mask = wo.pack_mask(wo.gate_bit(gx.cpu(), sc.cpu(), sh.cpu())).to(dev)
                    coef = torch.stack([torch.rand(k, generator=g) + 0.5, torch.randn(k, generator=g) * 0.2, torch.randn(k, generator=g) * 0.3,
                                        torch.randn(k, generator=g) * 0.1]).to(dev).contiguous()
                    with ops.large_batch_dispatch() as disp, ops.arithmetic(arith):
                        put(what, "fwd", ops.wino_conv2d_fwd(x, w)[0])
                        y, part, _ = ops.wino_conv2d_fwd(x, w, want_stats=True)
                        put(what, "fwd_stats.y", y), put(what, "fwd_stats.pmean", part[0]), put(what, "fwd_stats.pm2", part[1])
                        out[f"wino_chain/{arith}/{what}/fwd_stats.rows_per_group"] = np.int64(part[2])
                        put(what, "fwd_affine", ops.wino_conv2d_fwd(x, w, in_affine=(sc, sh))[0])
                        y, _, v = ops.wino_conv2d_fwd(x, w, keep_v=True)
                        put(what, "fwd_keep_v.y", y), put(what, "fwd_keep_v.v", v)
                        put(what, "dgrad", ops.wino_conv2d_dgrad(dy, w))
                        for tag, gate in (("affine", ops.BnGateCtx(gx, mean, invstd, scale=sc, shift=sh)), ("mask", ops.BnGateCtx(gx, mean, invstd, mask=mask))):
                            dx = ops.wino_conv2d_dgrad(dy, w, gate=gate)
                            put(what, f"dgrad_{tag}.dx", dx), put(what, f"dgrad_{tag}.psum_g", dx._gate_partials[0]), put(what, f"dgrad_{tag}.psum_gx", dx._gate_partials[1])
                        for acc in (0, 1):
                            dw = rn(k, c, 3, 3, scale=0.1).contiguous(memory_format=torch.channels_last)
                            d2 = dy.clone()
                            ops.wino_conv2d_wgrad(v, d2, w, dw, accumulate=bool(acc))
                            put(what, f"wgrad_acc{acc}", dw)
                        put(what, "dgrad_after_wgrad", ops.wino_conv2d_dgrad(d2, w))          # F(4x4): picks up the transformed input the one pass over dy left
                        if off is None and v.shape[0] == 36:
                            lazy, dw = ops.LazyGrad(dy, rn(n, h, w_, k), coef), torch.zeros_like(w)
                            ops.wino_conv2d_wgrad(v, lazy, w, dw, accumulate=False)
                            put(what, "lazy.wgrad", dw), put(what, "lazy.dgrad", ops.wino_conv2d_dgrad(lazy, w))
                    out[f"wino_chain/{arith}/{what}/dispatch"] = np.frombuffer(json.dumps(disp.log, sort_keys=True).encode(), dtype=np.uint8)
        finally:
            if off:
                setattr(ops, off, prev)


def dump(path, chain):
    """the child: every case in both arithmetics on the library SSV_HIP_LIB names -> one .npz of raw arrays, keyed family/arithmetic/case/output"""
    import torch
    import densecl_oracle as do
    import nnclr_oracle as no
    import pcl_oracle as po
    import test_gpu_bn_pool_kernels as bp
    import test_gpu_dense_nce_forms as qn
    import test_gpu_nn_lookup_forms as nn
    import test_gpu_proto_nce_forms as pn
    import test_gpu_vit_kernels as vk
    import test_gpu_wino_forms as wf
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
    dev = torch.device("cuda:0")
    for case in wf.CASES:
        if case.kind in wf.CALLERS:
            for k, v in wf.CALLERS[case.kind][0](case, wf.Run(case, dev)).items():
                out[f"wino_stage/{case.id}/{k}"] = v.cpu().numpy() if torch.is_tensor(v) else np.int64(v)
    for case in vk.CASES:
        if case.kind in ("afwd", "abwd", "acomp"):
            ctx = vk.Ctx(dev)
            got = vk.GPU[case.kind](case, vk.KINDS[case.kind][1](case), ctx)
            ctx.verify(case.id)
            for k, v in got.items():
                out[f"attention/{case.id}/{k}"] = v.detach().cpu().numpy()
    for case in bp.CASES:
        ctx = bp.Ctx(dev)
        got = bp.GPU[case.kind](case, bp.KINDS[case.kind][1](case), ctx)
        ctx.verify(case.id)
        for k, v in got.items():
            a = v.detach().cpu().numpy()
            if a.nbytes > BIG_BYTES:
                a = np.frombuffer(json.dumps({"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "shape": list(a.shape), "dtype": str(a.dtype)}).encode(), dtype=np.uint8)
            out[f"bn_pool/{case.id}/{k}"] = a
        del ctx, got
    if chain:
        from ssv_amd import ops
        for arith in ARITHS:
            chains(ops, dev, arith, out)
    np.savez(path, **out)
    print("SHA " + _lib.source_sha16())


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old", nargs="?")
    ap.add_argument("new", nargs="?")
    ap.add_argument("-o", "--out")
    ap.add_argument("--old-root", help="a checkout of the parent commit: the old library's child imports the package from it, and both children run the chain table")
    ap.add_argument("--dump", help=argparse.SUPPRESS)
    ap.add_argument("--chain", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.dump:
        dump(a.dump, a.chain)
        return 0
    assert a.old and a.new, "two libraries to compare"
    shas, dumps, seconds = {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, lib in (("parent", a.old), ("new", a.new)):
            path = os.path.join(tmp, tag + ".npz")
            t0 = time.time()
            try:
                env = dict(os.environ, SSV_HIP_LIB=os.path.abspath(lib), SSV_SAME_BITS_ROOT=os.path.abspath(a.old_root) if (a.old_root and tag == "parent") else ROOT)
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", path] + (["--chain"] if a.old_root else []), env=env,
                                     capture_output=True, text=True, timeout=CHILD_SECONDS)
            except subprocess.TimeoutExpired:
                sys.stderr.write(f"the child on {lib} ran into its time limit of {CHILD_SECONDS} s: nothing more is run\n")
                return 2
            if res.returncode != 0:
                sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:] + f"\nthe child on {lib} failed (rc {res.returncode}): nothing more is run\n")
                return 2
            seconds[tag] = round(time.time() - t0, 1)
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
                   "C-ABI calls of the forms tests in both arithmetics; the dumped arrays (loss, lse, dq, flag; the lookup: idx, sim, nn; the Winograd stages: every "
                   "array their runners return and the host answers; attention: every afwd, abwd and acomp case of tests/test_gpu_vit_kernels.CASES through its "
                   "guarded callers, every array they return; BatchNorm and pooling: every case of tests/test_gpu_bn_pool_kernels.CASES through its guarded "
                   "runners, every tensor they return (above 16 MB: its sha256, shape and dtype); with --old-root the chain table through ops.wino_conv2d_* with the old child's package taken "
                   "from the parent's tree: every result, partial, kept V and the dispatch log) are compared byte for byte",
           "old_root": bool(a.old_root),
           "ssv_source_sha16": shas, "child_seconds": seconds, "child_time_limit": CHILD_SECONDS, "cases_compared": len(cases), "all_identical": ok, "cases": cases}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    for case, e in cases.items():
        if not e["identical"]:
            print(f"DIFFERENT {case}: {e['differs']}")
    print(f"{len(cases)} cases, {sum(e['identical'] for e in cases.values())} identical; parent {shas['parent']} ({seconds['parent']} s), new {shas['new']} ({seconds['new']} s)")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
