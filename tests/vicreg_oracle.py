"""The VICReg loss (Bardes, Ponce, LeCun 2022, the paper's pseudocode) as plain torch lines, parameterised by dtype (float64 is the reference, the SAME lines in
float32 give ref32), the closed-form gradient csrc/vicreg.hip implements, the case table of tests/test_vicreg_cpu.py and tests/test_gpu_vicreg.py, and the CPU
generator of their inputs, seeded by the case id.

    sim  = mean over B*D of (x - y)^2
    xc   = x - mean_b(x);  s_x = sqrt(var_unbiased(x, dim 0) + eps)                      (y likewise)
    std  = mean_j relu(1 - s_x[j]) / 2 + mean_j relu(1 - s_y[j]) / 2
    C_x  = xc^T xc / (B - 1);  cov = sum_{i != j} C_x[i][j]^2 / D + sum_{i != j} C_y[i][j]^2 / D
    loss = sim_coeff * sim + std_coeff * std + cov_coeff * cov

The hinge has a kink at s = 1: columns are randn times a per-column scale that alternates between 0.25 and 4.0, so the hinge is active on half the columns
and no s[j] sits near 1 (test_vicreg_cpu.py asserts |s[j] - 1| > 0.05 for every column of every case).  Coefficients and eps enter as the fp32 numbers the
C ABI's float arguments carry (``f32``).
"""
import zlib
from collections import namedtuple

import torch

EPS = 1e-4
DEFAULT = (25.0, 25.0, 1.0)
HINGE_MARGIN = 0.05

# scales: "alt" = 0.25 / 4.0 alternating by column, or one number for every column; shift: added to every element; coeffs: the (sim, std, cov) triples the case runs
Case = namedtuple("Case", "B D scales shift coeffs")

CASES = {
    "tiny": Case(8, 32, "alt", 0.0, (DEFAULT,)),                          # one strip, one trip of every loop
    "ragged_rows": Case(37, 64, "alt", 0.0, (DEFAULT,)),                  # B not a multiple of the row step
    "strips": Case(64, 160, "alt", 0.0, (DEFAULT,)),                      # several column strips, D not a multiple of 64
    "two_rows": Case(2, 32, "alt", 0.0, (DEFAULT,)),                      # the smallest legal batch, B - 1 = 1
    "offset_mean": Case(64, 128, "alt", 100.0, (DEFAULT,)),               # E[x^2] - mean^2 would lose every digit here
    "trips": Case(1500, 256, "alt", 0.0, (DEFAULT,)),                     # further trips of the row loop and of the D x D reduction
    "config": Case(512, 2048, "alt", 0.0, (DEFAULT,)),                    # the shipped width
    "all_active": Case(64, 128, 0.25, 0.0, (DEFAULT,)),                   # hinge active everywhere
    "none_active": Case(64, 128, 4.0, 0.0, (DEFAULT,)),                   # hinge nowhere active: std term exactly 0
    "weights": Case(64, 128, "alt", 0.0, ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))),      # each term alone
}


def f32(v):
    """a scalar as the C ABI's float argument carries it"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def runs():
    """(run id, case name, coefficient triple) for every evaluation of the table"""
    out = []
    for name, c in CASES.items():
        for k, co in enumerate(c.coeffs):
            out.append((name if len(c.coeffs) == 1 else f"{name}{k}", name, co))
    return out


def column_scales(case):
    if case.scales == "alt":
        return torch.tensor([0.25, 4.0]).repeat(case.D // 2)
    return torch.full((case.D,), float(case.scales))


def generate(name):
    """x, y [B, D] fp32 from a CPU generator seeded by the case id: y is x plus a tenth of its column scale of noise (two views of one sample)."""
    c = CASES[name]
    gen = torch.Generator().manual_seed(zlib.crc32(("vicreg." + name).encode()))
    sc = column_scales(c)
    z = torch.randn(c.B, c.D, generator=gen)
    if c.B < 4:                              # a handful of rows has no typical spread: standardise the draw, so that a column's std IS its scale and stays off the kink
        z = (z - z.mean(dim=0)) / z.std(dim=0)
    x = z * sc
    y = x + 0.1 * torch.randn(c.B, c.D, generator=gen) * sc
    return (x + c.shift).contiguous(), (y + c.shift).contiguous()


def loss_lines(x, y, sim_coeff, std_coeff, cov_coeff, eps):
    """The paper's lines.  Returns (loss, (weighted sim, std, cov terms), intermediates)."""
    b, d = x.shape
    sim = ((x - y) ** 2).mean()
    xc, yc = x - x.mean(dim=0), y - y.mean(dim=0)
    sx, sy = torch.sqrt(xc.pow(2).sum(dim=0) / (b - 1) + eps), torch.sqrt(yc.pow(2).sum(dim=0) / (b - 1) + eps)
    std = torch.relu(1 - sx).mean() / 2 + torch.relu(1 - sy).mean() / 2
    craw_x, craw_y = xc.t() @ xc, yc.t() @ yc
    cx, cy = craw_x / (b - 1), craw_y / (b - 1)
    off = 1 - torch.eye(d, dtype=x.dtype)
    cov = (cx * off).pow(2).sum() / d + (cy * off).pow(2).sum() / d
    terms = (sim_coeff * sim, std_coeff * std, cov_coeff * cov)
    loss = terms[0] + terms[1] + terms[2]
    return loss, terms, {"xc": torch.stack((xc, yc)), "s": torch.stack((sx, sy)), "craw": torch.stack((craw_x, craw_y))}


def closed_form(x, y, sim_coeff, std_coeff, cov_coeff, eps):
    """The gradient as csrc/vicreg.hip forms it, in x's dtype: e (the sim and std terms), G (the scaled off-diagonal covariance) and d = xc G + e per view."""
    b, d = x.shape
    _, _, mid = loss_lines(x, y, sim_coeff, std_coeff, cov_coeff, eps)
    xc, s, craw = mid["xc"], mid["s"], mid["craw"]
    g_sim = 2 * sim_coeff * (x - y) / (b * d)
    sim_term = torch.stack((g_sim, -g_sim))
    active = (s < 1).to(x.dtype)
    std_term = -std_coeff / (2 * d * (b - 1)) * xc * (active / s).unsqueeze(1)
    off = 1 - torch.eye(d, dtype=x.dtype)
    g = 4 * cov_coeff / (d * (b - 1) ** 2) * craw * off
    cov_term = xc @ g
    return {"sim_term": sim_term, "std_term": std_term, "cov_term": cov_term, "e": sim_term + std_term, "G": g, "d": cov_term + sim_term + std_term}


def cgrad_lines(craw, b, cov_coeff, parts, dtype):
    """What ssv_vicreg_cgrad makes of a given craw [2, D, D] and parts [2] (fp32 inputs), in `dtype`: (G, loss [4])."""
    craw, parts = craw.to(dtype), parts.to(dtype)
    d = craw.shape[1]
    off = 1 - torch.eye(d, dtype=dtype)
    g = 4 * cov_coeff / (d * (b - 1) ** 2) * craw * off
    cov = cov_coeff * ((craw / (b - 1) * off).pow(2).sum() / d)
    return g, torch.stack((parts[0] + parts[1] + cov, parts[0], parts[1], cov))


def reference(run_id, name, coeffs, dtype):
    """Everything the kernels and the loss module produce, in `dtype`, gradients by autograd.  Results are cached: compute once, share, leave unchanged."""
    key = (run_id, name, tuple(coeffs), dtype)
    if key in _REF:
        return _REF[key]
    x32, y32 = generate(name)
    sc, st, cv = (f32(v) for v in coeffs)
    eps = f32(EPS)
    x, y = x32.to(dtype).requires_grad_(True), y32.to(dtype).requires_grad_(True)
    loss, terms, mid = loss_lines(x, y, sc, st, cv, eps)
    loss.backward()
    with torch.no_grad():
        cf = closed_form(x.detach(), y.detach(), sc, st, cv, eps)
    out = {"xc": mid["xc"].detach(), "s": mid["s"].detach(), "craw": mid["craw"].detach(), "e": cf["e"], "G": cf["G"],
           "loss": torch.stack([loss.detach()] + [t.detach() for t in terms]), "dx": x.grad, "dy": y.grad}
    _REF[key] = out
    return out


_REF = {}


def errors(x, ref64):
    """e(x) = |x - ref64|_2 / |ref64|_2 and m(x) = max|x - ref64| / max|ref64| (tests/test_gpu_loss_kernels.py, rule (a)); 0 / 0 counts as 0"""
    d = x.to(torch.float64) - ref64
    n, mx = float(torch.linalg.vector_norm(ref64)), float(ref64.abs().max())
    dn, dm = float(torch.linalg.vector_norm(d)), float(d.abs().max())
    return (dn / n if n > 0 else (0.0 if dn == 0 else float("inf"))), (dm / mx if mx > 0 else (0.0 if dm == 0 else float("inf")))
