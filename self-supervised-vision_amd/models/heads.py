"""Projector / predictor heads of the three accelerated algorithms, composed from the HIP ops.
Parameter names, shapes and init draws follow the reference so state_dicts and seeds interchange:
  SimCLR ProjectionHead  models/simclr.py:23-36   fc1 bn1 fc2 bn2
  BYOL   MLP             models/byol.py:24-34     fc1 bn1 fc2
  Barlow ProjectionHead  models/barlow.py:23-36   layer1.{0,1} layer2.{0,1} layer3, then L2-normalise
  VICReg ProjectionHead  (not in the reference)   Barlow's three layers without the final L2 normalisation
  NNCLR  Projection/PredictionHead  (not in the reference)   layer1.{0,1} layer2.{0,1} layer3.{0,1}  /  layer1.{0,1} layer2
  W-MSE  ProjectionHead  (not in the reference)   layer1.{0,1} layer2, not normalised
  DenseCL DenseProjectionHead  (not in the reference)   layer1.{0,1} layer2 on the rows of the feature map
"""
import math

import torch
import torch.nn as nn

from .. import nn as hnn
from .. import ops


def _fresh_linear(din, dout):
    """nn.Linear's default init: kaiming_uniform_(weight, a=sqrt 5) then bias ~ U(-1/sqrt(fan_in), +)."""
    w = torch.empty(dout, din)
    nn.init.kaiming_uniform_(w, a=math.sqrt(5))
    bound = 1.0 / math.sqrt(din)
    b = torch.empty(dout)
    nn.init.uniform_(b, -bound, bound)
    return hnn.HipLinear(din, dout, weight=w, bias=b)


class SimclrProjectionHead(hnn.HipModule):
    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.fc1 = _fresh_linear(input_dim, input_dim)
        self.bn1 = hnn.HipBatchNorm(input_dim)
        self.fc2 = _fresh_linear(input_dim, output_dim)
        self.bn2 = hnn.HipBatchNorm(output_dim)

    def _run(self, tape, x):
        x = hnn.batchnorm(tape, self.fc1._run(tape, x), self.bn1, relu=True)
        return hnn.batchnorm(tape, self.fc2._run(tape, x), self.bn2)


class ByolMLP(hnn.HipModule):
    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.fc1 = _fresh_linear(input_dim, input_dim)
        self.bn1 = hnn.HipBatchNorm(input_dim)
        self.fc2 = _fresh_linear(input_dim, output_dim)

    def _run(self, tape, x):
        return self.fc2._run(tape, hnn.batchnorm(tape, self.fc1._run(tape, x), self.bn1, relu=True))


class _LinearBnRelu(nn.Sequential):
    def __init__(self, din, dout):
        super().__init__(_fresh_linear(din, dout), hnn.HipBatchNorm(dout))     # the reference's third entry (ReLU) has no state

    def _run(self, tape, x):
        return hnn.batchnorm(tape, self[0]._run(tape, x), self[1], relu=True)


class BarlowProjectionHead(hnn.HipModule):
    def __init__(self, input_dim, projection_dim):
        super().__init__()
        self.layer1 = _LinearBnRelu(input_dim, projection_dim)
        self.layer2 = _LinearBnRelu(projection_dim, projection_dim)
        self.layer3 = _fresh_linear(projection_dim, projection_dim)

    def _run(self, tape, x):
        x = self.layer2._run(tape, self.layer1._run(tape, x))
        return hnn.l2_normalize(tape, self.layer3._run(tape, x))


class _LinearBn(nn.Sequential):
    def __init__(self, din, dout):
        super().__init__(_fresh_linear(din, dout), hnn.HipBatchNorm(dout))

    def _run(self, tape, x):
        return hnn.batchnorm(tape, self[0]._run(tape, x), self[1])


class NnclrProjectionHead(hnn.HipModule):
    """NNCLR's projector (Dwibedi et al. 2021, section 4.1): Linear-BN-ReLU, Linear-BN-ReLU, Linear-BN.  The loss normalises its output."""

    def __init__(self, input_dim, hidden_dim, output_dim):
        super().__init__()
        self.layer1 = _LinearBnRelu(input_dim, hidden_dim)
        self.layer2 = _LinearBnRelu(hidden_dim, hidden_dim)
        self.layer3 = _LinearBn(hidden_dim, output_dim)

    def _run(self, tape, x):
        return self.layer3._run(tape, self.layer2._run(tape, self.layer1._run(tape, x)))


class NnclrPredictionHead(hnn.HipModule):
    """NNCLR's predictor: Linear-BN-ReLU, Linear, back to the projector's width."""

    def __init__(self, dim, hidden_dim):
        super().__init__()
        self.layer1 = _LinearBnRelu(dim, hidden_dim)
        self.layer2 = _fresh_linear(hidden_dim, dim)

    def _run(self, tape, x):
        return self.layer2._run(tape, self.layer1._run(tape, x))


def _narrow_linear(tape, x, lin):
    """hnn.linear for a layer whose output is narrower than the data-gradient kernels take (they contract over Dout in steps of 16): forward and weight gradient are
    the usual launches, the data gradient runs on dy and the weight padded with zero columns / rows to the next multiple of 16."""
    weight, bias = lin.weight, lin.bias
    b, din = x.shape
    dout = weight.shape[0]
    x4 = x.view(b, 1, 1, din)
    y = ops.conv2d_fwd(x4, weight, 1, 0, bias=bias).view(b, dout)
    if tape is not None:
        need_dx, slot = tape.needs_grad(x), tape.slot

        def bwd(dy, existing):
            ops.conv2d_wgrad(x4, dy.view(b, 1, 1, dout), weight, hnn.grad_of(weight, slot), 1, 0, accumulate=True, dbias=hnn.grad_of(bias, slot))
            if not need_dx:
                return (None,)
            kp = (dout + 15) // 16 * 16
            wp = torch.zeros((kp, din), dtype=torch.float32, device=x.device)
            wp[:dout].copy_(weight.detach())
            ex = existing[0]
            ex4 = None if ex is None else ex.view(b, 1, 1, din)
            dx = ops.conv2d_dgrad(ops.pad_channels(dy.contiguous(), kp).view(b, 1, 1, kp), wp, x4.shape, 1, 0, addend=ex4, out=ex4)
            ops.drop_planes(wp)                  # the padded copy is no weight: its bf16 planes must not wait in the cache for the next optimizer step
            return (dx.view(b, din),)
        tape.record((x,), y, bwd)
    return y


class WmseProjectionHead(hnn.HipModule):
    """W-MSE's projector (Ermolov et al. 2021, section 5): Linear-BN-ReLU, Linear.  The whitening fixes the scale of the output, so nothing is normalised.  The
    embedding may be as narrow as 4 columns (the whitening's smallest width): see _narrow_linear."""

    def __init__(self, input_dim, hidden_dim, output_dim):
        super().__init__()
        self.layer1 = _LinearBnRelu(input_dim, hidden_dim)
        self.layer2 = _fresh_linear(hidden_dim, output_dim)
        self.narrow = output_dim % 16 != 0

    def _run(self, tape, x):
        h = self.layer1._run(tape, x)
        return _narrow_linear(tape, h, self.layer2) if self.narrow else self.layer2._run(tape, h)


class DenseProjectionHead(hnn.HipModule):
    """DenseCL's dense projector on the rows [B * cells, C] of the final feature map (the paper's 1x1 conv - ReLU - 1x1 conv, which on rows is two Linear
    layers): layer1 = Linear(C, C)-BN-ReLU, layer2 = Linear(C, D).  The paper's head has no BatchNorm; the heads of this project are built on the fused BN + ReLU
    kernel and there is no stand-alone ReLU, so layer1 carries one (its statistics run over all cells of the batch).  The loss normalises the output."""

    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.layer1 = _LinearBnRelu(input_dim, input_dim)
        self.layer2 = _fresh_linear(input_dim, output_dim)

    def _run(self, tape, x):
        return self.layer2._run(tape, self.layer1._run(tape, x))


class VicregProjectionHead(BarlowProjectionHead):
    """VICReg's expander: the loss works on the raw embeddings (its variance term fixes their scale), so nothing is normalised."""

    def _run(self, tape, x):
        return self.layer3._run(tape, self.layer2._run(tape, self.layer1._run(tape, x)))
