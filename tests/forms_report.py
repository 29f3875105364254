"""TEST INFRASTRUCTURE shared by tests/test_gpu_kmeans_forms.py and tests/test_gpu_pirl_forms.py: rule (a) of tests/test_gpu_loss_kernels.py for one family of
outputs, guarded device buffers, and the report both files write into under SSV_KMEANS_PIRL_REPORT=<path> (profiles/kmeans_pirl_forms_report.json).  The
nearest-neighbour lookup, ProtoNCE and whitening form tests share it too and write profiles/lookup_loss_forms_report.json under SSV_LOOKUP_LOSS_FORMS_REPORT.
The DenseCL form tests (tests/test_gpu_dense_nce_forms.py, tests/test_gpu_dense_match_forms.py) write a third report, profiles/densecl_forms_report.json, under
SSV_DENSECL_FORMS_REPORT.  The augmentation form tests (tests/test_gpu_augment_forms.py) take the guarded buffers alone: they compare bits, not errors, and write
profiles/augment_forms_report.json themselves.

Rule (a): with ref64 the plain reference in float64, ref32 the SAME lines in float32, e(x) = ||x - ref64||_2 / ||ref64||_2 and m(x) = max|x - ref64| / max|ref64|,
    e(got) <= FACTOR * e(ref32) + FLOOR     and the same for m;
e(ref32) comes from the reference alone.  FACTOR is the worst max(0, e(got) - FLOOR) / e(ref32) (and m) measured on an MI355X over every case of the family,
rounded up to the next power of two and never above 8; FLOOR is at most 16 * 2^-24."""
import json
import math
import os

import numpy as np
import torch

U = 2.0 ** -24
GUARD = 1024                                                             # elements behind (and, for the bank, in front of) every buffer a kernel writes
SENTINEL = -77                                                           # the guard of an integer buffer
NAN_BITS = 0x7FC00000                                                    # a float NaN as an int32 prefill
GARBAGE = 0x5A5A5A5A                                                     # 1.5e16 as a float, 1515870810 as an int32


def errors(x, ref64):
    """(e, m) of the docstring; numpy arrays or torch tensors (or scalars) of any float type."""
    x = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, np.float64).reshape(-1)
    r = np.asarray(ref64.detach().cpu() if isinstance(ref64, torch.Tensor) else ref64, np.float64).reshape(-1)
    d = x - r
    return float(np.sqrt((d * d).sum()) / max(np.sqrt((r * r).sum()), 1e-300)), float(np.abs(d).max() / max(np.abs(r).max(), 1e-300))


def ratio(got, ref, floor):
    if got <= floor:
        return 0.0
    return (got - floor) / ref if ref > 0 else float("inf")


def next_pow2(r):
    return 1.0 if r <= 1.0 else 2.0 ** math.ceil(math.log2(r))


class Family:
    """One (FACTOR, FLOOR) pair and the figures measured under it."""

    def __init__(self, name, factor, floor):
        self.name, self.factor, self.floor, self.cases = name, factor, floor, {}

    def hold(self, what, name, got, ref64, ref32, fails):
        """Record and print the figures of one output, then append to `fails` when it misses rule (a) (the caller asserts once everything is printed)."""
        (eg, mg), (er, mr) = errors(got, ref64), errors(ref32, ref64)
        self.cases.setdefault(what, {})[name] = {"e_got": eg, "e_ref32": er, "m_got": mg, "m_ref32": mr}
        print(f"{what} {name}: e {eg:.3e} (ref32 {er:.3e}) m {mg:.3e} (ref32 {mr:.3e})")
        if not (eg <= self.factor * er + self.floor and mg <= self.factor * mr + self.floor):
            fails.append(f"{what} {name}: e {eg:.3e} vs ref32 {er:.3e}, m {mg:.3e} vs ref32 {mr:.3e} (FACTOR {self.factor:g}, FLOOR {self.floor:.2e})")

    def summary(self):
        out = {"FACTOR": self.factor, "FLOOR": self.floor, "worst_e_ratio": 0.0, "worst_m_ratio": 0.0, "worst_e_case": "", "worst_m_case": ""}
        for what, tensors in self.cases.items():
            for name, r in tensors.items():
                for k in ("e", "m"):
                    v = ratio(r[f"{k}_got"], r[f"{k}_ref32"], self.floor)
                    if v > out[f"worst_{k}_ratio"]:
                        out[f"worst_{k}_ratio"], out[f"worst_{k}_case"] = v, f"{what} {name}"
        out["FACTOR_implied"] = min(8.0, next_pow2(max(out["worst_e_ratio"], out["worst_m_ratio"])))
        return out


def write(families, env="SSV_KMEANS_PIRL_REPORT", sha_key="ssv_source_sha16", extra=None):
    """Merge the families measured by this process into the report the environment variable `env` names (the test files of one report write one file between
    them; by default the k-means / PIRL one).  `extra`: further top-level entries, merged key by key."""
    path = os.environ.get(env)
    if not path:
        return
    from ssv_amd import _lib
    doc = {"families": {}, "cases": {}}
    if os.path.exists(path):
        with open(path) as fh:
            doc = json.load(fh)
    doc[sha_key] = _lib.source_sha16()
    for fam in families:
        if fam.cases:
            doc["families"][fam.name] = fam.summary()
            doc["cases"][fam.name] = fam.cases
    for key, value in (extra or {}).items():
        if value:
            doc.setdefault(key, {}).update(value)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)


class Buffers:
    """Device buffers with GUARD elements behind them: outputs prefilled with a value the kernel cannot produce, inputs kept to prove them untouched."""

    def __init__(self):
        self.guarded, self.inputs = [], []

    def out(self, name, n, dtype, prefill, front=False):
        guard = float("nan") if dtype.is_floating_point else SENTINEL
        lead = GUARD if front else 0
        buf = torch.full((lead + n + GUARD,), guard, dtype=dtype, device="cuda")
        buf[lead:lead + n] = prefill
        self.guarded.append((name, buf, lead, n))
        return buf[lead:lead + n]

    def up(self, name, a, dtype=None):
        d = torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a, dtype=dtype).contiguous().cuda()
        self.inputs.append((name, d, d.clone()))
        return d

    def verify(self, what):
        torch.cuda.synchronize()
        for name, d, keep in self.inputs:
            assert torch.equal(bits(d), bits(keep)), f"{what}: input {name} was modified"
        for name, buf, lead, n in self.guarded:
            for g in (buf[:lead], buf[lead + n:]):
                ok = torch.isnan(g).all() if buf.is_floating_point() else (g == SENTINEL).all()
                assert bool(ok), f"{what} {name}: wrote outside its buffer"


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
