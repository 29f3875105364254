"""GPU: every launch form of csrc/pirl.hip - ssv_pirl_loss_fwd_bwd, ssv_bank_momentum_update and ssv_patch_split straight through the C ABI - against
tests/pirl_oracle.py evaluated on the CPU in float64 (ref64) and in float32 (ref32): po.pirl_loss on bank[pos] and bank[neg], po.bank_update, po.patches.
Temperatures, weights and momenta enter both references as the fp32 values the kernel receives.  The inputs are po.loss_case_inputs with a seed per case.

Held for the loss: rule (a) of tests/test_gpu_loss_kernels.py (tests/forms_report.py) on the loss, d_img and d_patch by both e and m, family pirl.loss (a
gradient whose reference is identically zero - a loss weight of 0 or 1 - must be exactly zero instead); loss, d_img and d_patch are NaN-prefilled views with
1024 floats of guard behind them; the workspace is ssv_pirl_loss_workspace_bytes(B, 64) bytes as the header prescribes, 256-byte aligned, guarded and holding
garbage before the call; every input is bit-identical afterwards; a second call - with the other workspace prefill - gives equal bits; the flag word (the first
int32 of the workspace) is zero for every case whose indices are valid.  Both `normalize` values are run unless the row says otherwise.  tests/test_pirl_cpu.py
shows that every case is well conditioned and keeps this table honest.

Branch labels (label, entry point, what the case reaches); loss shapes are (B, D, K, N):

  lse.k1             ssv_pirl_loss_fwd_bwd     (5, 32, 1, 16): one negative, 31 masked columns of the only tile
  lse.k_edge         ssv_pirl_loss_fwd_bwd     (33, 32, 31 / 32 / 33, 200): K tail masked; B one past a row block
  lse.b_edge         ssv_pirl_loss_fwd_bwd     (1 / 31 / 32, 64, 70, 200): row-block edges
  lse.width          ssv_pirl_loss_fwd_bwd     D = 4, 8, 12, 36, 68, 128, 508, 512 at (40, D, 70, 300): the half-step guard 8 q + 4 h < D with and without the upper half-step, lda with and without the pad column, the d += 64 trips of pirl_rows_k
  lse.split_ragged   ssv_pirl_loss_fwd_bwd     (40, 32, 320, 600), splits 4: 10 tiles -> 3 + 3 + 3 + 1, the last split has three idle waves
  lse.split_thin     ssv_pirl_loss_fwd_bwd     the same, splits 10: one tile per split, three idle waves everywhere
  lse.split_clamp    ssv_pirl_loss_fwd_bwd     (40, 32, 70, 300), splits 64: a request above the 3 tiles
  lse.split_max      ssv_pirl_loss_fwd_bwd     (40, 32, 2100, 4000), splits 64: 66 tiles -> 2 per split -> 33 effective splits ("no empty split")
  lse.split_default  ssv_pirl_loss_fwd_bwd     splits 0 is bit-identical to passing ssv_pirl_default_splits(B, K): every case that leaves the split to the library
  lse.online_max     ssv_pirl_loss_fwd_bwd     bank rows scaled by 6, normalize 0, T 0.05: logits of several hundred - the max subtraction in the tile sweep, the half-wave merge, the wave merge and the split merge
  lse.weight_edge    ssv_pirl_loss_fwd_bwd     loss_weight 0 and 1: the side with zero weight gets exact zeros in its gradient
  lse.bad_neg        ssv_pirl_loss_fwd_bwd     (40, 32, 70, 300) with neg[3] = -1, neg[40] = N, neg[69] = 2^40: masked out - held to the references on the remaining 67 negatives, flag non-zero
  lse.bad_tile       ssv_pirl_loss_fwd_bwd     the same with ALL of neg[32:64] out of range: a whole tile masked (tmax == -inf leaves the running pair untouched)
  lse.bad_pos        ssv_pirl_loss_fwd_bwd     pos[0] = N: flag non-zero, every output finite, rows 1.. of d_img / d_patch bit-identical to the run with the valid index; the loss value of that row is not pinned; run once
  bank.width         ssv_bank_momentum_update  N 50, n 9, D = 4, 32, 68, 128, 512: one, partial and many trips of the lane loops
  bank.n_edge        ssv_bank_momentum_update  n = 1, 4, 5: the four-rows-per-workgroup edge
  bank.init          ssv_bank_momentum_update  momentum 0 on a zero bank: initialize_vectors
  bank.skip          ssv_bank_momentum_update  one index -1 and one N among valid ones: skipped, every other row as without them, bit for bit
  bank.zero_row      ssv_bank_momentum_update  an all-zero feature row, eps 1e-12: the row only shrinks - m * old, finite
  patch.tall         ssv_patch_split           (B, H, W, C, patch) = (2, 32, 16, 3, 8): H / patch != W / patch, the x-outside-y order is observable
  patch.wide         ssv_patch_split           (3, 16, 48, 64, 16): the other way round
  patch.whole        ssv_patch_split           (1, 8, 8, 4, 8): a single patch is the whole image

The bank is a view with guards on BOTH sides, its indices are distinct (the ABI requires it), rows not named are bit-unchanged; bank rows under rule (a),
family pirl.bank, against po.bank_update.  The patch split is an exact permutation: torch.equal against po.patches, output guarded.

FACTOR / FLOOR: see below and profiles/kmeans_pirl_forms_report.json.
"""
import re

import pytest
import torch

import forms_report as fr
import pirl_oracle as po

U = fr.U
# by the rule of tests/forms_report.py from the MI355X run committed as profiles/kmeans_pirl_forms_report.json: worst ratios 4.33 (pirl.loss: m of d_img at
# lse.b_edge B 31, normalize 0) and 0 (pirl.bank: every case within the floor)
FACTOR = {"pirl.loss": 8.0, "pirl.bank": 1.0}
FLOOR = {"pirl.loss": 2 * U, "pirl.bank": 2 * U}                        # the final rounding of an fp32 result, twice where a prior is added (the bank row)
FAMILIES = {name: fr.Family(name, FACTOR[name], FLOOR[name]) for name in FACTOR}
COND = 1e-3


def _s(x):
    """a scalar as the C ABI's float argument carries it"""
    return float(torch.tensor(float(x), dtype=torch.float32))


class Case:
    def __init__(self, labels, b, d, k, n, splits=0, normalize=(1, 0), temperature=0.2, weight=0.3, scale=1.0, bad=None):
        self.labels, self.shape, self.splits, self.normalize, self.temperature, self.weight, self.scale, self.bad = \
            tuple(labels.split()), (b, d, k, n), splits, normalize, temperature, weight, scale, bad
        self.id = f"{self.labels[0]}-{b}x{d}x{k}x{n}-s{splits}-w{weight:g}" + (f"-{bad}" if bad else "")


_SPLIT = " lse.split_default"
CASES = [Case("lse.k1" + _SPLIT, 5, 32, 1, 16)]
CASES += [Case("lse.k_edge" + _SPLIT, 33, 32, k, 200) for k in (31, 32, 33)]
CASES += [Case("lse.b_edge" + _SPLIT, b, 64, 70, 200) for b in (1, 31, 32)]
CASES += [Case("lse.width" + _SPLIT, 40, d, 70, 300) for d in (4, 8, 12, 36, 68, 128, 508, 512)]
CASES += [
    Case("lse.split_ragged", 40, 32, 320, 600, splits=4),
    Case("lse.split_thin", 40, 32, 320, 600, splits=10),
    Case("lse.split_clamp", 40, 32, 70, 300, splits=64),
    Case("lse.split_max", 40, 32, 2100, 4000, splits=64),
    Case("lse.online_max lse.split_ragged", 40, 32, 320, 600, splits=4, normalize=(0,), temperature=0.05, scale=6.0, weight=0.5),
    Case("lse.online_max" + _SPLIT, 40, 32, 320, 600, normalize=(0,), temperature=0.05, scale=6.0, weight=0.5),
    Case("lse.weight_edge" + _SPLIT, 40, 32, 70, 300, weight=0.0),
    Case("lse.weight_edge" + _SPLIT, 40, 32, 70, 300, weight=1.0),
    Case("lse.bad_neg" + _SPLIT, 40, 32, 70, 300, bad="neg"),
    Case("lse.bad_tile" + _SPLIT, 40, 32, 70, 300, bad="tile"),
    Case("lse.bad_pos" + _SPLIT, 40, 32, 70, 300, normalize=(1,), bad="pos"),
]
BANK_CASES = [("bank.width", dict(N=50, n=9, D=d, m=0.9)) for d in (4, 32, 68, 128, 512)]
BANK_CASES += [("bank.n_edge", dict(N=50, n=n, D=128, m=0.5)) for n in (1, 4, 5)]
BANK_CASES += [("bank.init", dict(N=50, n=9, D=128, m=0.0, zero_bank=True)), ("bank.skip", dict(N=50, n=9, D=128, m=0.5, skip=True)),
               ("bank.zero_row", dict(N=50, n=9, D=128, m=0.5, zero_row=3))]
PATCH_CASES = [("patch.tall", (2, 32, 16, 3, 8)), ("patch.wide", (3, 16, 48, 64, 16)), ("patch.whole", (1, 8, 8, 4, 8))]


def documented_labels():
    out = {}
    for line in __doc__.splitlines():
        m = re.match(r"^  ([a-z0-9_]+\.[a-z0-9_]+)\s+(ssv_\w+)\s+\S", line)
        if m:
            out[m.group(1)] = m.group(2)
    return out


def plan(k, splits):
    """(tiles, tiles per split, effective splits) of ssv_pirl_loss_fwd_bwd for a positive request, restated."""
    tiles = (k + 31) // 32
    splits = max(1, min(splits, tiles, 64))
    per = -(-tiles // splits)
    return tiles, per, -(-tiles // per)


def loss_inputs(case):
    """(img, patch, bank, pos, neg) fp32 / int64 CPU tensors; the case's out-of-range indices are in place."""
    b, d, k, n = case.shape
    img, patch, bank, pos, neg = po.loss_case_inputs(b, d, k, n, 3000 + 10 * CASES.index(case))
    bank = bank * case.scale
    if case.bad in ("neg", "tile"):
        neg[3], neg[40], neg[69] = -1, n, 2 ** 40
    if case.bad == "tile":
        neg[32:64] = torch.where(torch.arange(32) % 2 == 0, n + torch.arange(32), -1 - torch.arange(32))
    if case.bad == "pos":
        pos[0] = n
    return img, patch, bank, pos, neg


def loss_reference(case, inp, dtype, normalize):
    """{"loss", "d_img", "d_patch"} in `dtype`: po.pirl_loss on bank[pos] and the bank rows of the negatives that lie inside the bank."""
    img, patch, bank, pos, neg = inp
    zi, zp = img.to(dtype).clone().requires_grad_(), patch.to(dtype).clone().requires_grad_()
    rows = bank.to(dtype)
    inside = neg[(neg >= 0) & (neg < rows.shape[0])]
    loss = po.pirl_loss(zi, zp, rows[pos], rows[inside], bool(normalize), 1.0 / _s(1.0 / case.temperature), _s(case.weight))
    loss.backward()
    return {"loss": loss.detach(), "d_img": zi.grad, "d_patch": zp.grad}


def bank_inputs(position):
    """(bank [N, D], index [n] distinct, z [n, D]) fp32 / int64 CPU tensors of BANK_CASES[position]."""
    _, p = BANK_CASES[position]
    bank = torch.zeros(p["N"], p["D"]) if p.get("zero_bank") else po.randn(3500 + 3 * position, p["N"], p["D"])
    index = torch.randperm(p["N"], generator=torch.Generator().manual_seed(3501 + 3 * position))[:p["n"]].clone()
    z = po.randn(3502 + 3 * position, p["n"], p["D"]) * 1.7
    if p.get("zero_row") is not None:
        z[p["zero_row"]] = 0.0
    return bank, index, z


def bank_reference(bank, index, z, momentum, dtype):
    out = bank.to(dtype).clone()
    po.bank_update(out, index, z.to(dtype), _s(momentum))
    return out


# ====================================================================================================================== GPU side
@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from ssv_amd import _lib
    yield _lib.load()
    fr.write(list(FAMILIES.values()))


def _loss_gpu(lib, case, inp, normalize, splits, ws_fill, what):
    from ssv_amd import _lib
    P = _lib.ptr
    b, d, k, n = case.shape
    buf = fr.Buffers()
    img, patch, bank, pos, neg = (buf.up(nm, t) for nm, t in zip(("img", "patch", "bank", "pos", "neg"), inp))
    loss = buf.out("loss", 1, torch.float32, float("nan"))
    d_img, d_patch = (buf.out(nm, b * d, torch.float32, float("nan")).view(b, d) for nm in ("d_img", "d_patch"))
    nbytes = lib.ssv_pirl_loss_workspace_bytes(b, 64)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = buf.out("ws", nbytes // 4, torch.int32, ws_fill)
    assert ws.data_ptr() % 256 == 0 and bank.data_ptr() % 16 == 0
    _lib.call("ssv_pirl_loss_fwd_bwd", n, d, b, k, P(bank), P(pos), P(neg), P(img), P(patch), int(normalize), 1.0 / case.temperature, case.weight, splits,
              P(loss), P(d_img), P(d_patch), P(ws), nbytes, _lib.stream())
    buf.verify(what)
    out = {"loss": loss.clone(), "d_img": d_img.clone(), "d_patch": d_patch.clone()}
    for name, t in out.items():
        assert bool(torch.isfinite(t).all()), f"{what} {name}: elements never written, or not finite"
    return out, int(ws[0])


def _same(a, b, what):
    for name in a:
        assert torch.equal(fr.bits(a[name]), fr.bits(b[name])), f"{what}: {name} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_loss_forms_against_fp64(lib, case):
    inp = loss_inputs(case)
    b, d, k, n = case.shape
    fails = []
    for normalize in case.normalize:
        what = f"{case.id} normalize {normalize}"
        got, flag = _loss_gpu(lib, case, inp, normalize, case.splits, fr.NAN_BITS, what)
        again, flag2 = _loss_gpu(lib, case, inp, normalize, case.splits, fr.GARBAGE, what + " (second call)")
        _same(got, again, what + ": two calls")
        assert (flag != 0) == (case.bad is not None) and (flag2 != 0) == (flag != 0), f"{what}: flag word {flag}"
        if case.splits == 0:
            default = lib.ssv_pirl_default_splits(b, k)
            assert default >= 1
            named, _ = _loss_gpu(lib, case, inp, normalize, default, fr.NAN_BITS, what + f" (splits {default})")
            _same(got, named, what + ": splits 0 against the default named")
        if case.bad == "pos":
            valid = list(inp)
            valid[3] = po.loss_case_inputs(b, d, k, n, 3000 + 10 * CASES.index(case))[3]
            assert valid[3][0] != inp[3][0] and torch.equal(valid[3][1:], inp[3][1:])
            ref, flag = _loss_gpu(lib, case, valid, normalize, case.splits, fr.NAN_BITS, what + " (valid index)")
            assert flag == 0
            print(f"{what}: loss {float(got['loss']):.6f} with the index outside the bank, {float(ref['loss']):.6f} with it inside")
            for name in ("d_img", "d_patch"):
                assert torch.equal(fr.bits(got[name])[1:], fr.bits(ref[name])[1:]), f"{what}: rows 1.. of {name} differ from the run with the valid index"
            continue
        r64, r32 = loss_reference(case, inp, torch.float64, normalize), loss_reference(case, inp, torch.float32, normalize)
        for name, ref64 in r64.items():
            if not float(ref64.abs().max()) > 0:
                assert name == ("d_patch" if case.weight == 0.0 else "d_img") and case.weight in (0.0, 1.0)
                assert bool((got[name] == 0).all()), f"{what} {name}: not exactly zero under a zero weight"
                continue
            FAMILIES["pirl.loss"].hold(what, name, got[name], ref64, r32[name], fails)
    assert not fails, "\n".join(fails)


def _bank_gpu(bank, index, z, momentum, eps, what):
    from ssv_amd import _lib
    P = _lib.ptr
    buf = fr.Buffers()
    n_rows, d = bank.shape
    dev = buf.out("bank", n_rows * d, torch.float32, bank.reshape(-1).cuda(), front=True).view(n_rows, d)
    idx, zd = buf.up("index", index), buf.up("z", z)
    _lib.call("ssv_bank_momentum_update", n_rows, d, P(dev), index.numel(), P(idx), P(zd), momentum, eps, _lib.stream())
    buf.verify(what)
    return dev.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("position", range(len(BANK_CASES)), ids=lambda i: f"{BANK_CASES[i][0]}-{i}")
def test_bank_update_forms_against_fp64(lib, position):
    label, p = BANK_CASES[position]
    bank, index, z = bank_inputs(position)
    what = f"{label} {p}"
    call_index = index.clone()
    if p.get("skip"):
        call_index[2], call_index[6] = -1, p["N"]
    got = _bank_gpu(bank, call_index, z, p["m"], 1e-12, what)
    inside = (call_index >= 0) & (call_index < p["N"])
    rows = call_index[inside]
    r64, r32 = (bank_reference(bank, rows, z[inside], p["m"], dt) for dt in (torch.float64, torch.float32))
    assert bool(torch.isfinite(got).all())
    untouched = torch.ones(p["N"], dtype=torch.bool)
    untouched[rows] = False
    assert torch.equal(fr.bits(got)[untouched], fr.bits(bank)[untouched]), f"{what}: a row that was not named changed"
    fails = []
    FAMILIES["pirl.bank"].hold(what, "bank rows", got[rows], r64[rows], r32[rows], fails)
    if p.get("skip"):
        without = _bank_gpu(bank, rows, z[inside], p["m"], 1e-12, what + " (without the skipped entries)")
        assert torch.equal(fr.bits(got), fr.bits(without)), f"{what}: the skipped entries changed another row"
    if p.get("zero_row") is not None:
        row = index[p["zero_row"]]
        assert torch.equal(fr.bits(got[row]), fr.bits(torch.tensor(p["m"], dtype=torch.float32) * bank[row])), f"{what}: the zero feature did more than shrink its row"
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("position", range(len(PATCH_CASES)), ids=lambda i: PATCH_CASES[i][0])
def test_patch_split_forms_are_the_reference_slices(lib, position):
    from ssv_amd import _lib
    P = _lib.ptr
    label, (b, h, w, c, ps) = PATCH_CASES[position]
    x = po.randn(3700 + position, b, c, h, w)
    want = po.patches(x, ps)
    count = (h // ps) * (w // ps)
    assert len(want) == count and (label == "patch.whole") == (count == 1) and (label == "patch.whole" or h // ps != w // ps)
    buf = fr.Buffers()
    xd = buf.up("x", x.permute(0, 2, 3, 1).contiguous())
    out = buf.out("patches", count * b * ps * ps * c, torch.float32, float("nan")).view(count, b, ps, ps, c)
    _lib.call("ssv_patch_split", b, h, w, c, ps, P(xd), P(out), _lib.stream())
    buf.verify(label)
    got = out.cpu().permute(0, 1, 4, 2, 3)
    for p, slices in enumerate(want):
        assert torch.equal(got[p], slices), f"{label}: patch {p}"
