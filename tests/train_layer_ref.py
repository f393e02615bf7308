"""A plain float64 restatement of ONE conv + BatchNorm layer of the training step (forward, running-statistic update and
backward), for tests/test_train_layers.py to hold every layer of `DIMTrainer.backward` against at batch sizes no CPU
oracle runs a whole MobileNetV2 at, and for tests/test_train_layers_cpu.py to pin to torch's own conv2d / batch_norm /
autograd.

Torch code that runs on any device, from matmuls, slices, elementwise operations and reductions only (no `conv2d`, no
`batch_norm`), so that the device path needs nothing but float64 matmul and elementwise kernels.  Activations are NHWC
`[B, H, W, C]` (the layout the training step keeps them in); weights have the reference's state_dict shapes (stem
`[32, C, 3, 3]`, depthwise `[c, 1, 3, 3]`, pointwise `[cout, cin, 1, 1]`).  Every input is up-cast to float64.

  kind "stem"  3x3, stride 2, padding 1, C inputs     a [M, 9 C] @ [9 C, cout] matmul over nine shifted slices
  kind "dw"    depthwise 3x3, stride 1 or 2, padding 1  nine shifted, strided slices of the zero-padded input x tap weights
  kind "pw"    pointwise                               [M, cin] @ W.T
"""
from typing import List, NamedTuple, Optional

import torch

from oatomobile_amd import arch

BN_MOMENTUM = 0.1  # nn.BatchNorm2d's default
F64 = torch.float64


class LayerSpec(NamedTuple):
  """One row of `layer_table`: what a check of conv layer `index` needs to know."""
  index: int
  kind: str       # "stem" | "dw" | "pw"
  conv: str       # state_dict prefix of the conv (its weight is conv + ".weight")
  bn: str         # state_dict prefix of its BatchNorm
  cin: int
  cout: int
  h_in: int
  h_out: int
  stride: int
  relu6: bool
  res_from: int   # the layer whose post-activation is added to this layer's output (a residual projection), or -1


def _bn_prefix(conv: str) -> str:
  head, last = conv.rsplit(".", 1)
  return "%s.%d" % (head, int(last) + 1)


def layer_table(in_channels: int = 2) -> List[LayerSpec]:
  """The conv layers of the network in `arch.conv_layers` order (the index `DIMTrainer.peek` takes), with the input
  width, stride and residual source that `arch.blocks` implies."""
  names = arch.conv_layers(in_channels)
  rows = [("stem", in_channels, arch.INPUT_HW, 2, -1)]
  for b in arch.blocks():
    first = len(rows)
    if b.expand:
      rows.append(("pw", b.inp, b.h_in, 1, -1))
    rows.append(("dw", b.hidden, b.h_in, b.stride, -1))
    rows.append(("pw", b.hidden, b.h_out, 1, first - 1 if b.residual else -1))
  rows.append(("pw", arch.INVERTED_RESIDUAL_SETTING[-1][1], names[-1].h_out, 1, -1))
  assert len(rows) == len(names)
  out = []
  for i, ((kind, cin, h_in, stride, res), n) in enumerate(zip(rows, names)):
    assert (h_in if kind == "pw" else arch.conv_out(h_in, stride)) == n.h_out, (i, n)
    assert kind != "dw" or cin == n.cout
    out.append(LayerSpec(i, kind, n.name, _bn_prefix(n.name), cin, n.cout, h_in, n.h_out, stride, n.relu6, res))
  return out


# ------------------------------------------------------------------------------------------------------------------
# convolutions and their adjoints
# ------------------------------------------------------------------------------------------------------------------
def _out_hw(h: int, stride: int) -> int:
  return (h + 2 - 3) // stride + 1


def _pad(x: torch.Tensor) -> torch.Tensor:
  B, H, W_, C = x.shape
  xp = x.new_zeros(B, H + 2, W_ + 2, C)
  xp[:, 1:H + 1, 1:W_ + 1, :] = x
  return xp


def _tap(xp: torch.Tensor, dy: int, dx: int, ho: int, wo: int, stride: int) -> torch.Tensor:
  """The view of the padded input that tap (dy, dx) of every output pixel reads."""
  return xp[:, dy:dy + stride * (ho - 1) + 1:stride, dx:dx + stride * (wo - 1) + 1:stride, :]


def _stem_matrix(W: torch.Tensor) -> torch.Tensor:
  """[cout, C, 3, 3] -> [9 C, cout], rows ordered (dy, dx, c) like `_patches`."""
  return W.permute(2, 3, 1, 0).reshape(-1, W.shape[0])


def _patches(x: torch.Tensor, stride: int) -> torch.Tensor:
  B, H, W_, C = x.shape
  ho, wo = _out_hw(H, stride), _out_hw(W_, stride)
  xp = _pad(x)
  return torch.cat([_tap(xp, dy, dx, ho, wo, stride) for dy in range(3) for dx in range(3)], dim=-1)


def conv_forward(kind: str, x: torch.Tensor, W: torch.Tensor, stride: int = 1) -> torch.Tensor:
  """`pre` [B, Ho, Wo, cout] of the conv of NHWC `x` with `W`."""
  x, W = x.to(F64), W.to(F64)
  B, H, W_, C = x.shape
  if kind == "pw":
    return (x.reshape(-1, C) @ W.reshape(W.shape[0], C).t()).reshape(B, H, W_, W.shape[0])
  ho, wo = _out_hw(H, stride), _out_hw(W_, stride)
  if kind == "stem":
    return (_patches(x, stride).reshape(-1, 9 * C) @ _stem_matrix(W)).reshape(B, ho, wo, W.shape[0])
  assert kind == "dw", kind
  xp = _pad(x)
  out = x.new_zeros(B, ho, wo, C)
  for dy in range(3):
    for dx in range(3):
      out.addcmul_(_tap(xp, dy, dx, ho, wo, stride), W[:, 0, dy, dx])
  return out


def conv_weight_grad(kind: str, x: torch.Tensor, dpre: torch.Tensor, stride: int = 1) -> torch.Tensor:
  """dLoss/dW in W's state_dict shape, from the layer's input and dLoss/dpre."""
  x, dpre = x.to(F64), dpre.to(F64)
  B, H, W_, C = x.shape
  cout = dpre.shape[-1]
  if kind == "pw":
    return (dpre.reshape(-1, cout).t() @ x.reshape(-1, C)).reshape(cout, C, 1, 1)
  ho, wo = dpre.shape[1], dpre.shape[2]
  if kind == "stem":
    g = _patches(x, stride).reshape(-1, 9 * C).t() @ dpre.reshape(-1, cout)  # [9 C, cout]
    return g.reshape(3, 3, C, cout).permute(3, 2, 0, 1).contiguous()
  assert kind == "dw", kind
  xp = _pad(x)
  g = x.new_zeros(C, 1, 3, 3)
  for dy in range(3):
    for dx in range(3):
      g[:, 0, dy, dx] = (_tap(xp, dy, dx, ho, wo, stride) * dpre).sum(dim=(0, 1, 2))
  return g


def conv_input_grad(kind: str, dpre: torch.Tensor, W: torch.Tensor, stride: int, h_in: int, w_in: Optional[int] = None) -> torch.Tensor:
  """dLoss/dx [B, h_in, w_in, cin] from dLoss/dpre and the weights."""
  dpre, W = dpre.to(F64), W.to(F64)
  w_in = h_in if w_in is None else w_in
  B, ho, wo, cout = dpre.shape
  if kind == "pw":
    cin = W.shape[1]
    return (dpre.reshape(-1, cout) @ W.reshape(cout, cin)).reshape(B, ho, wo, cin)
  if kind == "stem":
    C = W.shape[1]
    dpatch = (dpre.reshape(-1, cout) @ _stem_matrix(W).t()).reshape(B, ho, wo, 9 * C)
    dxp = dpre.new_zeros(B, h_in + 2, w_in + 2, C)
    for k in range(9):
      _tap(dxp, k // 3, k % 3, ho, wo, stride).add_(dpatch[..., k * C:(k + 1) * C])
    return dxp[:, 1:h_in + 1, 1:w_in + 1, :].contiguous()
  assert kind == "dw", kind
  dxp = dpre.new_zeros(B, h_in + 2, w_in + 2, cout)
  for dy in range(3):
    for dx in range(3):
      _tap(dxp, dy, dx, ho, wo, stride).addcmul_(dpre, W[:, 0, dy, dx])
  return dxp[:, 1:h_in + 1, 1:w_in + 1, :].contiguous()


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm + activation + residual
# ------------------------------------------------------------------------------------------------------------------
def batch_statistics(pre: torch.Tensor):
  """(mean, biased variance, rows) per channel of NHWC `pre`, in float64."""
  flat = pre.to(F64).reshape(-1, pre.shape[-1])
  mean = flat.mean(dim=0)
  var = ((flat - mean)**2).mean(dim=0)
  return mean, var, flat.shape[0]


def _normaliser(pre, running_mean, running_var, batch_stats):
  if batch_stats:
    mean, var, _ = batch_statistics(pre)
  else:
    mean, var = running_mean.to(F64), running_var.to(F64)
  return mean, 1.0 / torch.sqrt(var + arch.BN_EPS)


def bn_act_forward(pre, gamma, beta, running_mean, running_var, batch_stats: bool, relu6: bool, residual=None):
  """(post, running_mean', running_var'): nn.BatchNorm2d (batch statistics: biased variance, eps 1e-5, and the running
  statistics move by momentum 0.1 towards the batch mean and the UNBIASED batch variance; `batch_stats=False`
  normalises with the running values and leaves them alone), then ReLU6 if `relu6`, then `+ residual`."""
  pre = pre.to(F64)
  rm, rv = running_mean.to(F64), running_var.to(F64)
  mean, invstd = _normaliser(pre, rm, rv, batch_stats)
  post = (pre - mean) * invstd * gamma.to(F64) + beta.to(F64)
  if relu6:
    post = post.clamp(0.0, 6.0)
  if residual is not None:
    post = post + residual.to(F64)
  if batch_stats:
    _, var, M = batch_statistics(pre)
    unbiased = var * M / (M - 1) if M > 1 else var
    rm = (1.0 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean
    rv = (1.0 - BN_MOMENTUM) * rv + BN_MOMENTUM * unbiased
  return post, rm, rv


class LayerGrads(NamedTuple):
  dbeta: torch.Tensor       # [cout]  sum g
  dgamma: torch.Tensor      # [cout]  sum g xhat
  dW: torch.Tensor          # W's shape
  dx: Optional[torch.Tensor]  # [B, h_in, w_in, cin], None with need_dx=False
  dbeta_abs: torch.Tensor   # [cout]  sum |g|: the rounding scale of dbeta
  dgamma_abs: torch.Tensor  # [cout]  sum |g xhat|
  dpre: torch.Tensor        # [B, Ho, Wo, cout]


def layer_backward(kind, x, W, stride, pre, post_hip, dpost, gamma, running_mean, running_var, batch_stats: bool,
                   relu6: bool, need_dx: bool = True) -> LayerGrads:
  """The backward pass of one layer from dLoss/dpost.

  g = dpost * [0 < post_hip < 6] for a ReLU6 layer (the mask is the one the implementation under test decided, so both
  sides differentiate the same piecewise-linear function), g = dpost otherwise (a residual's `+ res` passes dpost on
  unchanged: the caller adds it to the block input's gradient).  Then dbeta = sum g, dgamma = sum g xhat, and
    dpre = gamma invstd (g - dbeta / M - xhat dgamma / M)   batch statistics
    dpre = gamma invstd g                                   running statistics ("frozen")
  and the conv's two adjoints."""
  x, pre, g = x.to(F64), pre.to(F64), dpost.to(F64)
  if relu6:
    g = g * ((post_hip > 0) & (post_hip < 6)).to(F64)
  mean, invstd = _normaliser(pre, running_mean, running_var, batch_stats)
  xhat = (pre - mean) * invstd
  dims = (0, 1, 2)
  gx = g * xhat
  dbeta, dgamma = g.sum(dim=dims), gx.sum(dim=dims)
  dbeta_abs, dgamma_abs = g.abs().sum(dim=dims), gx.abs().sum(dim=dims)
  del gx
  scale = gamma.to(F64) * invstd
  if batch_stats:
    M = pre.numel() // pre.shape[-1]
    dpre = (g - dbeta / M - xhat * (dgamma / M)) * scale
  else:
    dpre = g * scale
  del xhat, g
  dW = conv_weight_grad(kind, x, dpre, stride)
  dx = conv_input_grad(kind, dpre, W, stride, x.shape[1], x.shape[2]) if need_dx else None
  return LayerGrads(dbeta, dgamma, dW, dx, dbeta_abs, dgamma_abs, dpre)
