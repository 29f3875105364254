#!/usr/bin/env python3
"""Are two csrc trees the same machine code?  Compiles the device side of every .hip of the Makefile's SRCS in both trees to gfx950 assembly (the Makefile's
FLAGS + --cuda-device-only -S; no GPU needed) and compares, per kernel symbol, the sequence of instruction mnemonics (operands stripped, so register
renumbering passes) and the kernel's register / scratch / LDS metadata.
    python tools/isa_compare.py OLD_CSRC NEW_CSRC [-o report.json] [-j jobs]
One JSON entry per kernel: identical, instruction count, metadata; exit status 1 unless every kernel is identical."""
import argparse
import concurrent.futures
import json
import os
import re
import subprocess
import sys
import tempfile

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def make_var(csrc, name):
    out = subprocess.run(["make", "-s", "-C", csrc, "-pn", "print-src-sha"], capture_output=True, text=True).stdout
    return re.search(rf"^{name} :?= (.*)$", out, re.M).group(1).split()


def device_asm(csrc, src, flags, tmp, tag):
    out = os.path.join(tmp, f"{tag}_{src}.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", src, "-o", out], cwd=csrc, check=True, capture_output=True)
    return open(out).read()


def kernels(asm):
    """{symbol: (mnemonics, metadata)} of one device assembly file"""
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", asm)[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.symbol:\s+(\S+)\.kd", blk).group(1)
        meta[name] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", blk).group(1)) for k in META}
    res = {}
    for name, m in meta.items():
        body = re.search(rf"^{re.escape(name)}:.*?\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S).group(1)
        ops = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line or line.endswith(":") or line.startswith("."):
                continue
            ops.append(line.split()[0])
        res[name] = (ops, m)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-o", "--out")
    ap.add_argument("-j", "--jobs", type=int, default=8)
    a = ap.parse_args()
    srcs, flags = make_var(a.new, "SRCS"), make_var(a.new, "FLAGS")
    assert srcs == make_var(a.old, "SRCS") and flags == make_var(a.old, "FLAGS"), "the two trees build different sources or with different flags"
    report, ok = [], True
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        jobs = {(s, t): ex.submit(device_asm, d, s, flags, tmp, t) for s in srcs for t, d in (("old", a.old), ("new", a.new))}
        for s in srcs:
            old, new = kernels(jobs[s, "old"].result()), kernels(jobs[s, "new"].result())
            for name in sorted(set(old) | set(new)):
                o, n = old.get(name), new.get(name)
                same_ops, same_meta = bool(o and n and o[0] == n[0]), bool(o and n and o[1] == n[1])
                e = {"file": s, "kernel": name, "identical": same_ops and same_meta, "mnemonics_identical": same_ops, "metadata_identical": same_meta,
                     "instructions": {"old": len(o[0]) if o else None, "new": len(n[0]) if n else None},
                     "metadata": {"old": [o[1][k] for k in META] if o else None, "new": [n[1][k] for k in META] if n else None}}
                ok &= e["identical"]
                report.append(e)
    doc = {"flags": " ".join(flags + ["--cuda-device-only", "-S"]), "metadata_fields": list(META), "kernels": len(report), "all_identical": ok, "per_kernel": report}
    if a.out:
        with open(a.out, "w") as f:               # one line per kernel
            head = json.dumps({k: v for k, v in doc.items() if k != "per_kernel"}, indent=1)
            f.write(head[:-2] + ',\n "per_kernel": [\n  ' + ",\n  ".join(json.dumps(e) for e in report) + "\n ]\n}\n")
    for e in report:
        if not e["identical"]:
            print(f"DIFFERENT {e['file']} {e['kernel']} mnemonics={e['mnemonics_identical']} metadata={e['metadata_identical']} {e['instructions']}")
    print(f"{len(report)} kernels, {sum(e['identical'] for e in report)} identical")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
