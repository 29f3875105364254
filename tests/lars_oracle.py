"""The LARS update of csrc/lars.hip as plain torch lines, parameterised by dtype (float64 is the reference, the SAME lines in float32 give ref32), the case
table of tests/test_lars_cpu.py and tests/test_gpu_lars.py, and the CPU generator of their inputs, seeded by the case id.

Per tensor t with flags decay_t, adapt_t:
    u   = (g + g2) + (decay_t ? wd : 0) * p           (g2 absent: u = g + ...)
    q_t = eta * |p|_2 / |u|_2   if adapt_t and |p|_2 > 0 and |u|_2 > 0, else 1
    mu  = momentum * mu + q_t * u
    p   = p - lr * mu
lr / wd / momentum / eta enter as the fp32 numbers the kernel receives (``f32``).  Tensors sit in a flat arena the way utils/train_utils.ParamArena lays them
out: every tensor starts on a multiple of 64 floats, the floats between tensors are padding.
"""
import math
import zlib
from collections import namedtuple

import torch

ALIGN = 64                                                   # ParamArena's alignment, in floats
HYPER = {"lr": 0.3, "wd": 1e-4, "momentum": 0.9, "eta": 1e-3}

Case = namedtuple("Case", "shapes exclude two zero wd")
Layout = namedtuple("Layout", "shapes offsets numels total decay adapt")


def f32(x):
    """a scalar as four device floats carry it"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def cases(c):
    """The case table; c = ssv_lars_chunk_floats().  zero: tensor index -> which input is zeroed ('p', 'g' = g and g2, 'cancel' = g2 is -g)."""
    tiny = [(3,), (5, 7), (1,), (2, 3, 3, 2)]
    edges = [(c,), (c + 1,), (2 * c - 1,), (3, c), (64,), (10, 512), (10,)]
    sizes = [(1, 63, 64, 65, 1000)[i % 5] for i in range(200)]
    many = [(n,) if i % 2 else (1, n) for i, n in enumerate(sizes)]                         # every size both as a 1-D (excluded) and a 2-D (adapted) tensor
    return {
        "tiny": Case(tiny, True, True, {}, None),                                           # tails below a float4, a one-element tensor
        "chunk_edges": Case(edges, True, True, {}, None),                                   # first / last element of a chunk, a tensor that is exactly one chunk
        "many": Case(many, True, True, {}, None),                                           # tensor-table indexing beyond one wave or workgroup
        "big": Case([(512, 512, 3, 3), (2048,), (1000, 2048)], True, True, {}, None),       # hundreds of partials per tensor
        "zero_norms": Case([(40, 33), (7, 5, 3, 3), (130, 70)], True, True, {0: "p", 1: "g", 2: "cancel"}, 0.0),      # the q = 1 branches
        "no_exclusion": Case(tiny + edges, False, True, {}, None),                          # 1-D tensors adapted
        "one_view": Case(edges, True, False, {}, None),                                     # the single-slab form
    }


def layout(case):
    offsets, off = [], 0
    for s in case.shapes:
        offsets.append(off)
        off += (math.prod(s) + ALIGN - 1) // ALIGN * ALIGN
    on = [0 if (case.exclude and len(s) <= 1) else 1 for s in case.shapes]
    return Layout(case.shapes, offsets, [math.prod(s) for s in case.shapes], off, on, list(on))


def hyper(case):
    h = dict(HYPER)
    if case.wd is not None:
        h["wd"] = case.wd
    return {k: f32(v) for k, v in h.items()}


def generate(name, case):
    """p ~ N(0, 1 / fan_in), g, g2 ~ 1e-2 N(0, 1), mu ~ 1e-3 N(0, 1) per tensor, fp32, from a CPU generator seeded by the case id."""
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    out = []
    for i, s in enumerate(case.shapes):
        n = math.prod(s)
        fan_in = n // s[0] if len(s) > 1 else s[0]
        p = torch.randn(n, generator=gen) / math.sqrt(fan_in)
        g = 1e-2 * torch.randn(n, generator=gen)
        g2 = 1e-2 * torch.randn(n, generator=gen)
        mu = 1e-3 * torch.randn(n, generator=gen)
        z = case.zero.get(i)
        if z == "p":
            p.zero_()
        elif z == "g":
            g.zero_()
            g2.zero_()
        elif z == "cancel":
            g2 = -g
        out.append({"p": p, "g": g, "g2": g2 if case.two else None, "mu": mu})
    return out


def lars_tensor(p, g, g2, mu, decay, adapt, lr, wd, momentum, eta, dtype):
    """One LARS update of one tensor in `dtype`; returns (p, mu, q)."""
    p, g, mu = p.to(dtype), g.to(dtype), mu.to(dtype)
    u = (g + g2.to(dtype)) if g2 is not None else g
    u = u + (wd if decay else 0.0) * p
    pn, un = torch.linalg.vector_norm(p), torch.linalg.vector_norm(u)
    q = eta * pn / un if (adapt and pn > 0 and un > 0) else torch.ones((), dtype=dtype)
    mu = momentum * mu + q * u
    p = p - lr * mu
    return p, mu, q


def lars_step(tensors, decay, adapt, h, dtype):
    """One update of every tensor; returns the new tensor list (p, mu carried in `dtype`, the gradients kept) and the [T] ratios."""
    out, qs = [], []
    for t, d, a in zip(tensors, decay, adapt):
        p, mu, q = lars_tensor(t["p"], t["g"], t["g2"], t["mu"], d, a, h["lr"], h["wd"], h["momentum"], h["eta"], dtype)
        out.append({"p": p, "g": t["g"], "g2": t["g2"], "mu": mu})
        qs.append(q)
    return out, torch.stack(qs)


def reference(name, case, dtype):
    """(p, mu, q) after one step in `dtype`: p and mu concatenated over the tensors (no padding), q the [T] ratios.  float64 results are cached: compute once, share."""
    key = (name, dtype)
    if key not in _REF:
        lay = layout(case)
        out, q = lars_step(generate(name, case), lay.decay, lay.adapt, hyper(case), dtype)
        _REF[key] = (torch.cat([t["p"] for t in out]), torch.cat([t["mu"] for t in out]), q)
    return _REF[key]


_REF = {}


def errors(x, ref64):
    """e(x) = |x - ref64|_2 / |ref64|_2 and m(x) = max|x - ref64| / max|ref64| (tests/test_gpu_loss_kernels.py, rule (a))"""
    d = x.to(torch.float64) - ref64
    return float(torch.linalg.vector_norm(d) / torch.linalg.vector_norm(ref64)), float(d.abs().max() / ref64.abs().max())
