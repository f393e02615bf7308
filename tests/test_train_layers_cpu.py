"""tests/train_layer_ref.py is right: its written-out convolutions, BatchNorm and their adjoints against
`torch.nn.functional.conv2d` / `batch_norm` / `relu6` under autograd, in float64 on the CPU at B = 3, one layer of each
kind on the map sizes the real layer table uses.  Both sides are float64 evaluations of the same sums in a different
order: rtol 1e-11 per element, plus 1e-11 of the tensor's largest entry.  The second term is for the entries that cancel
to nothing: a float64 sum carries the rounding of its TERMS (1e-16 of them) whatever it adds up to, so with the relative
term alone 1 element in 22 500 of a stem's post-activations (value 2.5e-6 among values of 2, |difference| 1.0e-16) fails."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oatomobile_amd import arch
from tests import train_layer_ref as R

B = 3
RTOL = 1e-11

# (kind, cin, cout, h_in, stride, relu6, residual)
CASES = [
    pytest.param("stem", 2, 32, 100, 2, True, False, id="stem-C2-100to50"),
    pytest.param("stem", 4, 32, 100, 2, True, False, id="stem-C4-100to50"),
    pytest.param("stem", 2, 32, 9, 2, True, False, id="stem-C2-9to5"),
    pytest.param("dw", 12, 12, 50, 1, True, False, id="dw-s1-50"),
    pytest.param("dw", 12, 12, 13, 1, True, False, id="dw-s1-13"),
    pytest.param("dw", 12, 12, 4, 1, True, False, id="dw-s1-4"),
    pytest.param("dw", 12, 12, 50, 2, True, False, id="dw-s2-50to25"),
    pytest.param("dw", 12, 12, 25, 2, True, False, id="dw-s2-25to13"),
    pytest.param("dw", 12, 12, 13, 2, True, False, id="dw-s2-13to7"),
    pytest.param("dw", 12, 12, 7, 2, True, False, id="dw-s2-7to4"),
    pytest.param("pw", 16, 96, 13, 1, True, False, id="pw-relu6"),
    pytest.param("pw", 24, 8, 7, 1, False, False, id="pw-linear"),
    pytest.param("pw", 48, 8, 7, 1, False, True, id="pw-linear-residual"),
]


def _close(got, want, what):
  want = want.detach()
  np.testing.assert_allclose(got.detach().numpy(), want.numpy(), rtol=RTOL, atol=RTOL * float(want.abs().max()), err_msg=what)


def _torch_conv(kind, x_nchw, W, stride):
  if kind == "pw":
    return F.conv2d(x_nchw, W)
  return F.conv2d(x_nchw, W, stride=stride, padding=1, groups=x_nchw.shape[1] if kind == "dw" else 1)


@pytest.mark.parametrize("batch_stats", [True, False], ids=["train", "frozen"])
@pytest.mark.parametrize("kind,cin,cout,h_in,stride,relu6,residual", CASES)
def test_one_layer_vs_torch_autograd(kind, cin, cout, h_in, stride, relu6, residual, batch_stats):
  """Forward values (`conv_forward`, `bn_act_forward`), the running-statistic update and dbeta / dgamma / dW / dx of
  `layer_backward` from a random dLoss/dpost, against torch's own layer under autograd."""
  g = torch.Generator().manual_seed(7 + h_in + 100 * cin + stride)
  rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
  x = rnd(B, h_in, h_in, cin).requires_grad_(True)  # NHWC
  W = (rnd(cout, 1 if kind == "dw" else cin, *((1, 1) if kind == "pw" else (3, 3))) * 0.3).requires_grad_(True)
  gamma = (1.0 + 0.3 * rnd(cout)).requires_grad_(True)
  beta = (0.5 * rnd(cout)).requires_grad_(True)
  rm0, rv0 = 0.2 * rnd(cout), 0.5 + torch.rand(cout, generator=g, dtype=torch.float64)
  h_out = h_in if kind == "pw" else arch.conv_out(h_in, stride)
  res = rnd(B, h_out, h_out, cout) if residual else None
  dpost = rnd(B, h_out, h_out, cout)

  # torch's layer, NCHW
  rm_t, rv_t = rm0.clone(), rv0.clone()
  pre_t = _torch_conv(kind, x.permute(0, 3, 1, 2), W, stride)
  post_t = F.batch_norm(pre_t, rm_t, rv_t, gamma, beta, training=batch_stats, momentum=0.1, eps=arch.BN_EPS)
  if relu6:
    post_t = F.relu6(post_t)
  if res is not None:
    post_t = post_t + res.permute(0, 3, 1, 2)
  (post_t * dpost.permute(0, 3, 1, 2)).sum().backward()

  # the restatement, NHWC
  pre = R.conv_forward(kind, x.detach(), W.detach(), stride)
  assert pre.shape == (B, h_out, h_out, cout)
  _close(pre, pre_t.permute(0, 2, 3, 1), "pre")
  post, rm, rv = R.bn_act_forward(pre, gamma.detach(), beta.detach(), rm0, rv0, batch_stats, relu6, res)
  _close(post, post_t.permute(0, 2, 3, 1), "post")
  _close(rm, rm_t, "running_mean")
  _close(rv, rv_t, "running_var")
  if not batch_stats:
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
  else:
    assert float((rm - rm0).abs().max()) > 0
  if relu6:  # some elements on every branch of the clamp
    assert float((post == 0).double().mean()) > 0.02 and float(((post > 0) & (post < 6)).double().mean()) > 0.02
  out = R.layer_backward(kind, x.detach(), W.detach(), stride, pre, post, dpost, gamma.detach(), rm0, rv0, batch_stats, relu6)
  _close(out.dbeta, beta.grad, "dbeta")
  _close(out.dgamma, gamma.grad, "dgamma")
  _close(out.dW, W.grad, "dW")
  _close(out.dx, x.grad, "dx")
  assert out.dW.shape == W.shape and out.dx.shape == x.shape
  assert bool((out.dbeta_abs >= out.dbeta.abs()).all()) and bool((out.dgamma_abs >= out.dgamma.abs()).all())


def test_layer_table_follows_the_state_dict():
  """`layer_table`: 52 layers whose conv / BatchNorm prefixes and widths are the state_dict's, whose maps chain (a
  layer's input is the layer before it) and whose residual sources are the inputs of the ten residual blocks."""
  for C in (2, 4):
    table = R.layer_table(C)
    shapes = dict(arch.state_dict_spec(C))
    assert len(table) == 52 and [l.index for l in table] == list(range(52))
    for l in table:
      per_in = 1 if l.kind == "dw" else l.cin
      k = 1 if l.kind == "pw" else 3
      assert shapes[l.conv + ".weight"] == (l.cout, per_in, k, k), l
      for leaf in ("weight", "bias", "running_mean", "running_var"):
        assert shapes["%s.%s" % (l.bn, leaf)] == (l.cout,), l
      if l.index:
        prev = table[l.index - 1]
        assert (prev.cout, prev.h_out) == (l.cin, l.h_in), l
      if l.res_from >= 0:
        src = table[l.res_from]
        assert not l.relu6 and (src.cout, src.h_out) == (l.cout, l.h_out), l
    assert table[0].kind == "stem" and table[0].cin == C and table[0].h_in == arch.INPUT_HW
    assert sum(l.res_from >= 0 for l in table) == sum(b.residual for b in arch.blocks()) == 10
    assert sorted({(l.h_in, l.h_out) for l in table if l.kind == "dw" and l.stride == 2}) == [(7, 4), (13, 7), (25, 13), (50, 25)]
