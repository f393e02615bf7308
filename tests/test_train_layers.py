"""The DIM training step, layer by layer, against a float64 restatement at the batch sizes that change its launches.

`DIMTrainer.backward` picks its launch shapes from the batch size (csrc/train.hip: `gemm()`, `stat_grid()`, the
depthwise branch of `encoder_backward()`), and the oracle tests run it at B <= 12: observation groups in
`dw_wgrad_kernel`, split-K weight gradients of the 4x4 stage, the unsplit forward GEMMs of that stage and row blocks of
more than a thousand rows in the per-channel reductions are first reached at B = 64 .. 170.  Here one step runs at B = 69
and B = 277 (the smallest batches that reach those launch classes: `launch_classes` restates the host formulas and
asserts it), and EVERY one of the 52 conv layers and the head is checked on its own, teacher-forced on the tensors the
HIP step saved (`DIMTrainer.peek`): the layer's input, its pre-BatchNorm output, its ReLU6 decisions and its dLoss/dpost
are the HIP step's, the layer itself is tests/train_layer_ref.py in float64 on the device.  No kink decision and no
atomic ordering can move such a reference (tests/test_train_deterministic.py::decidable_case is what whole-step
comparisons have to do about that), and nothing the size of an activation arena crosses to the host.

Bounds (none of them taken from what the kernels give):
  forward (conv, BatchNorm + activation + residual)   |d| <= 1e-4 max|ref|: the suite's TOL, relative to the tensor
  running statistics (train)                          rtol 1e-4, atol 2e-6 (test_g15_train_step_vs_reference, step 0);
                                                      frozen: the same bits as before the step
  backward (dbeta, dgamma, dW, dx, head gradients)    |d| <= 2e-3 |ref| + 3e-4 max|ref| per element
                                                      (test_train_backward_vs_oracle_same_kinks, without its skip rule)
  dbeta, dgamma                                       ... + 1e-6 max_c sum|terms|: ~16 worst-case fp32 roundings of the
                                                      sum, so that the mathematically zero gradients (a BatchNorm bias in
                                                      front of another batch-statistics BatchNorm) are checked too
  z, loss                                             rtol 1e-4 / atol 2e-5, rtol 2e-5
A kernel that drops one observation of a ragged group, one row band or one K chunk is off by >= 1/277 = 3.6e-3 of the
tensor: twelve times the absolute term of the backward bound."""
import math
import time

import numpy as np
import pytest
import torch

from tests import train_layer_ref as R

pytestmark = pytest.mark.gpu

F64 = torch.float64


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------------------
# the host's launch decisions, restated (csrc/train.hip)
# ---------------------------------------------------------------------------------------------------------------------
def _ceil(a, b):
  return (a + b - 1) // b


def dw_wgrad_launch(B, cout, h_out):
  """`encoder_backward`, depthwise branch: (G observations per block, groups, row bands)."""
  chunks = (cout // 4 + 15) // 16
  G = max(1, min(8, B * chunks // 512))
  groups = _ceil(B, G)
  bands = max(1, min(h_out // 4, 1024 // (groups * chunks)))
  return G, groups, bands


def gemm_splits(ta, M, N, K):
  """`gemm()`: grid.z of a C[M,N] = A[M,K] B[K,N] call (1 = unsplit) and whether the last K chunk is ragged."""
  bn = 16 if (N <= 16 and M >= 256) else (32 if (N <= 32 and M >= 128) else 64)
  bm, bk = {16: 256, 32: 128, 64: 64}[bn], (16 if bn == 16 else 32)
  tiles = _ceil(N, bn) * _ceil(M, bm)
  if (K >= (1024 if ta else 4096) and tiles < 512) or (not ta and K >= 512 and tiles < 128):
    splits = min(_ceil(1024, tiles), _ceil(K, 256))
    if splits > 1:
      kchunk = _ceil(_ceil(K, splits), bk) * bk
      return _ceil(K, kchunk), K % kchunk != 0
  return 1, False


def stat_grid(M, C):
  """`stat_grid()`: (rows per block, row blocks) of the per-channel reduction kernels."""
  chunks = _ceil(C // 4, 16) if C % 4 == 0 else 1
  row_blocks = max(1, 512 // chunks)
  rpb = max(64, _ceil(M, row_blocks))
  return rpb, _ceil(M, rpb)


def launch_classes(B, C):
  """What batch B makes of the layer table, and the assertion that it is what the case is there for: retuning the host
  heuristics must fail here, not leave the cases running what B = 9 already runs."""
  table = R.layer_table(C)
  dw = [(l, dw_wgrad_launch(B, l.cout, l.h_out)) for l in table if l.kind == "dw"]
  Gs = {G for _, (G, _, _) in dw}
  ragged = {G for _, (G, _, _) in dw if G > 1 and B % G != 0}
  last = [l for l in table if l.kind == "pw" and l.h_out == table[-1].h_out]  # the 4x4 stage's pointwise layers
  fwd = [gemm_splits(False, B * l.h_out**2, l.cout, l.cin)[0] for l in last if l.cin >= 512]
  dgrad = [gemm_splits(False, B * l.h_out**2, l.cin, l.cout)[0] for l in last if l.cout >= 512]
  wgrad = [gemm_splits(True, l.cout, l.cin, B * l.h_out**2) for l in last]
  assert len(fwd) == 4 and len(dgrad) == 4 and len(last) == 8  # features.14's projection .. features.18
  stats = [stat_grid(B * l.h_out**2, l.cout) + (B * l.h_out**2,) for l in table]
  stem_blocks, stem_ragged = _ceil(B * table[0].h_out**2, 512), (B * table[0].h_out**2) % 512 != 0
  if B == 69:
    assert Gs == {1, 2} and ragged == {2}, (Gs, ragged)  # cout = 960: two observations per block, the last group has one
    assert all(z > 1 for z in fwd + dgrad), (fwd, dgrad)   # forward / input-gradient GEMMs of the 4x4 stage still split
  elif B == 277:
    assert Gs == {1, 3, 4, 8} and ragged == {3, 4, 8}, (Gs, ragged)
    assert any(l.stride == 2 and G > 1 for l, (G, _, _) in dw)
    assert all(z == 1 for z in fwd + dgrad), (fwd, dgrad)  # the path B = 128 and 512 take
    first = dw_wgrad_launch(B, table[1].cout, table[1].h_out)[2], dw_wgrad_launch(9, table[1].cout, table[1].h_out)[2]
    assert first == (3, 12), first  # the 50x50 maps drop from 12 row bands to 3
    assert any(rpb > 64 and M % rpb != 0 and gx > 256 for rpb, gx, M in stats)
    assert max(rpb for rpb, _, _ in stats) > 1024
  assert all(z > 1 and r for z, r in wgrad), wgrad  # the 4x4 stage's weight gradients split, kchunk ragged against K
  assert stem_blocks > 256 and stem_ragged
  return dict(G=sorted(Gs), fwd_splits=fwd, wgrad_splits=[z for z, _ in wgrad], stem_blocks=stem_blocks)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def visual_batch(B, C, dev, seed):
  """B synthetic BEVs with `tests/helpers.py:synth_observation`'s statistics, drawn as one array, through `transform`."""
  from oatomobile_amd import transform_visual
  rng = np.random.default_rng(seed)
  lidar = ((rng.integers(0, 6, size=(B, 200, 200, C)) / 5.0) * (rng.random((B, 200, 200, C)) < 0.12)).astype(np.float32)
  return transform_visual(torch.from_numpy(lidar).to(dev), channels_last=True)


def tail_batch(B, dev, seed):
  """The vector inputs, the target, its perturbed copy and a dropout keep mask."""
  from oatomobile_amd import arch
  rng = np.random.default_rng(seed)
  future = np.cumsum(np.abs(rng.normal(size=(B, arch.T, 2))) * 2.0, axis=1).astype(np.float32)
  batch = dict(velocity=torch.from_numpy(rng.normal(0, 3.0, size=(B, 3)).astype(np.float32)).to(dev),
               is_at_traffic_light=torch.from_numpy((rng.random((B, 1)) < 0.2).astype(np.float32)).to(dev),
               traffic_light_state=torch.from_numpy(rng.integers(0, 4, size=(B, 1)).astype(np.float32)).to(dev),
               player_future=torch.from_numpy(future).to(dev))
  y = torch.from_numpy(future + rng.normal(0, 1e-2, size=future.shape).astype(np.float32)).to(dev)
  keep = torch.from_numpy(((rng.random((B, arch.LAST_CHANNELS)) >= 0.2) / 0.8).astype(np.float32)).to(dev)
  return batch, y, keep


# ---------------------------------------------------------------------------------------------------------------------
# the head in float64: pool -> dropout -> classifier -> cat -> merger -> flow NLL (dim/model.py:203-217,
# sequence.py:153-216 as oracle/reference_cpu.py restates them), under torch autograd on the device
# ---------------------------------------------------------------------------------------------------------------------
HEAD_KEYS = ["_encoder._model.classifier.1.weight", "_encoder._model.classifier.1.bias"] + \
    ["_merger._model.%d.%s" % (2 * i, leaf) for i in range(3) for leaf in ("weight", "bias")] + \
    ["_decoder._decoder." + k for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + \
    ["_decoder._locscale._model.%d.%s" % (i, leaf) for i in (0, 2) for leaf in ("weight", "bias")]


def head_reference(post_last, keep, vec, y, sd, gradients=True):
  """(loss, z, smallest |pre-activation| of the ReLUs, {key: gradient}, dLoss/dpost of the last conv layer) from the NHWC
  post-activation of features.18."""
  p = {k: sd[k].to(F64).requires_grad_(gradients) for k in HEAD_KEYS}
  x = post_last.to(F64).requires_grad_(gradients)
  pooled = x.mean(dim=(1, 2)) * keep.to(F64)
  feat = pooled @ p[HEAD_KEYS[0]].t() + p[HEAD_KEYS[1]]
  h = torch.cat([feat, vec.to(F64)], dim=-1)
  margin = []
  for i in range(3):
    a = h @ p["_merger._model.%d.weight" % (2 * i)].t() + p["_merger._model.%d.bias" % (2 * i)]
    margin.append(a.detach().abs().min())
    h = torch.relu(a)
  z = h
  y = y.to(F64)
  H = z.shape[-1]
  w_ih, w_hh, b_ih, b_hh = (p["_decoder._decoder." + k] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
  y_prev = torch.zeros_like(y[:, 0, :])
  nll = 0.0
  for t in range(y.shape[1]):
    gi, gh = y_prev @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    u = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    h = (1.0 - u) * n + u * h
    a = h @ p["_decoder._locscale._model.0.weight"].t() + p["_decoder._locscale._model.0.bias"]
    margin.append(a.detach().abs().min())
    o = torch.relu(a) @ p["_decoder._locscale._model.2.weight"].t() + p["_decoder._locscale._model.2.bias"]
    scale = torch.nn.functional.softplus(o[:, 2:]) + 1e-3
    xt = (y[:, t, :] - (y_prev + o[:, :2])) / scale
    nll = nll + 0.5 * (xt**2).sum(-1) + math.log(2.0 * math.pi) + torch.log(scale).sum(-1)  # -(log_prob - logabsdet)
    y_prev = y[:, t, :]
  loss = nll.mean()
  if not gradients:
    return loss.detach(), z.detach(), torch.stack(margin).min(), None, None
  loss.backward()
  return loss.detach(), z.detach(), torch.stack(margin).min(), {k: v.grad for k, v in p.items()}, x.grad


# ---------------------------------------------------------------------------------------------------------------------
# the checks: every one leaves (family, name, deviation / bound, max|d| / max|ref|) as device scalars
# ---------------------------------------------------------------------------------------------------------------------
class Ledger:

  def __init__(self):
    self.rows = []

  def _add(self, family, name, d, bound, ref):
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bound).max()  # (0 / 0 = within; x / 0 = inf = outside)
    self.rows.append((family, name, ratio, d.max() / ref.abs().max().clamp_min(1e-300), ref.abs().max()))

  def forward(self, family, name, got, ref):
    """|d| <= 1e-4 max|ref|"""
    self._add(family, name, (got.to(F64) - ref).abs(), 1e-4 * ref.abs().max(), ref)

  def backward(self, family, name, got, ref, floor=None):
    """|d| <= 2e-3 |ref| + 3e-4 max|ref| (+ floor)"""
    bound = 2e-3 * ref.abs() + 3e-4 * ref.abs().max()
    self._add(family, name, (got.to(F64) - ref).abs(), bound if floor is None else bound + floor, ref)

  def allclose(self, family, name, got, ref, rtol, atol):
    self._add(family, name, (got.to(F64) - ref).abs(), atol + rtol * ref.abs(), ref)

  def settle(self, tag, nonzero_families):
    ratio = torch.stack([r[2] for r in self.rows]).cpu().numpy()
    rel = torch.stack([r[3] for r in self.rows]).cpu().numpy()
    scale = torch.stack([r[4] for r in self.rows]).cpu().numpy()
    worst = {}
    for (family, name, _, _, _), q, e in zip(self.rows, ratio, rel):
      if family not in worst or not q <= worst[family][0]:
        worst[family] = (float(q), name, float(e))
    for family, (q, name, e) in worst.items():
      print("%s %-8s worst deviation / bound %.3g (%s; max|d| / max|ref| there %.3g) over %d checks" %
            (tag, family, q, name, e, sum(r[0] == family for r in self.rows)))
    # a reference that is all zeros checks nothing (dbeta / dgamma may be mathematically zero: they have their floor)
    dead = [(r[0], r[1]) for r, s in zip(self.rows, scale) if r[0] in nonzero_families and not s > 0]
    assert not dead, dead
    bad = [(r[0], r[1], float(q)) for r, q in zip(self.rows, ratio) if not q <= 1.0]
    assert not bad, "%d of %d checks outside their bound (family, tensor, deviation / bound): %s" % (len(bad), len(self.rows), bad[:20])
    return worst


CASES = [
    pytest.param(69, 4, True, False, id="B69-C4-train"),
    pytest.param(69, 2, False, False, id="B69-C2-frozen"),
    pytest.param(277, 2, True, False, id="B277-C2-train"),
    pytest.param(277, 2, True, True, id="B277-C2-train-deterministic"),
]
KINK_MARGIN = 1e-5
SEEDS = 512  # B = 277 has 88 640 ReLU inputs in the head: about one tail in sixteen keeps them all 1.2e-5 from zero


@pytest.mark.parametrize("B,C,train,deterministic", CASES)
def test_every_layer_of_one_step_vs_float64(dev, B, C, train, deterministic):
  """One `DIMTrainer.backward` (replayed target and dropout mask, `max_batch` = B), then per conv layer, from the HIP
  step's own saved tensors: the conv, BatchNorm + ReLU6 + residual, the running statistics, dbeta / dgamma / dW and the
  gradient handed to the layer before (with the residual branch's second writer); and the head from features.18's
  post-activation: z, the loss, sixteen parameter gradients and the gradient handed to features.18.  Bounds: the module
  docstring.  The head's ReLUs (three in the merger, one per step in the flow's MLP) are its only kinks: the tail of the
  batch (vector inputs, target, mask) is the first of the seeds at which the float64 reference's smallest
  |pre-activation| exceeds 1.2e-5 (the selection looks at the reference alone), and the step that is checked must
  keep it above 1e-5, which is asserted.

  Measured on the MI355X (`pytest -s`; 434 checks a train case, 330 the frozen one; worst deviation / bound per family,
  in brackets the tensor's max|d| / max|ref|):
                  B = 69 C = 4 train   B = 69 frozen      B = 277 train      B = 277 deterministic
    conv          0.0060 (6.0e-7)      0.0071 (7.1e-7)    0.011 (1.1e-6)     0.011 (1.1e-6)
    bn-act        0.0028 (2.8e-7)      0.0021 (2.1e-7)    0.0033 (3.3e-7)    0.0033 (3.3e-7)
    running       0.0052               -                  0.0063             0.0063
    dbeta         0.022                0.00035            0.0092             0.0090
    dgamma        0.0053 (2.6e-6)      0.00037 (2.0e-7)   0.0069 (3.9e-6)    0.0054 (3.4e-6)
    dW            0.0023 (8.5e-7)      0.0012 (6.8e-7)    0.0039 (1.9e-6)    0.0042 (1.8e-6)
    dx            0.0011 (3.5e-7)      0.00068 (6.4e-7)   0.0016 (5.5e-7)    0.0014 (1.3e-6)
    head          0.011 (z 3.1e-7)     0.041 (z 3.2e-7)   0.014 (z 3.0e-7)   0.015 (z 2.9e-7)
  (the worst dbeta is features.17's projection bias, mathematically zero: 0.2-0.4 of its own largest entry and 1-2 %
  of the rounding floor it is held to).  Nothing is within a factor of 20 of its bound, where one dropped observation
  at B = 277 is twelve times over it.  The tail was the 1st seed at B = 69 and the 18th at B = 277 (margin 1.27e-5).
  Wall time per case, trainer construction and batch synthesis included: 4.6 / 3.4 / 3.9 / 3.8 s; the step, the tail
  selection and all checks: 1.15 / 0.39 / 0.64 / 0.63 s."""
  from oatomobile_amd import DIMTrainer, ImitativeModel, arch
  print("B=%d C=%d launch classes: %s" % (B, C, launch_classes(B, C)))
  table = R.layer_table(C)
  nl = len(table)
  tr = DIMTrainer(ImitativeModel.synthetic(41, in_channels=C).to(dev), lr=1e-3, max_batch=B, device=dev,
                  deterministic=deterministic)
  assert tr.deterministic == deterministic
  sd0 = tr.state_dict()  # clones: the parameters and running statistics the step starts from
  params0 = tr.params.clone()
  visual = visual_batch(B, C, dev, 5000 + B + C)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  nhwc = lambda i, what: tr.peek(i, what).permute(0, 2, 3, 1)  # the saved buffer itself: contiguous NHWC

  def step(tail, y, keep):
    tr.params.copy_(params0)  # (a train-mode step moves the running statistics inside `params`)
    tr.grads.fill_(float("nan"))  # every entry must be written by the step
    return tr.backward(dict(tail, visual_features=visual), y=y, dropout_mask=keep, train=train)

  # features.18's post-activation depends on the BEVs and the parameters alone: one step with any tail gives it, and the
  # tail is then chosen on the float64 head without running the HIP step again
  step(*tail_batch(B, dev, 6000))
  post_last = nhwc(nl - 1, "post")
  for seed in range(6000, 6000 + SEEDS):
    tail, y, keep = tail_batch(B, dev, seed)
    vec = torch.cat([tail["velocity"], tail["is_at_traffic_light"], tail["traffic_light_state"]], dim=-1)
    if float(head_reference(post_last, keep, vec, y, sd0, gradients=False)[2]) > 1.2 * KINK_MARGIN:
      break
  else:
    pytest.fail("no tail among %d seeds keeps the head's ReLUs %g from their kinks" % (SEEDS, 1.2 * KINK_MARGIN))
  loss = step(tail, y, keep)
  margin = float(head_reference(nhwc(nl - 1, "post"), keep, vec, y, sd0, gradients=False)[2])
  print("tail seed %d (%d tried): smallest |pre-activation| of the head's ReLUs in float64 %.3g" % (seed, seed - 5999, margin))
  assert margin > KINK_MARGIN, margin
  assert bool(torch.isfinite(tr.grads).all()) and bool(torch.isfinite(loss))
  sd1 = tr.state_dict()
  grads = tr.named_gradients()
  ledger = Ledger()

  # ---- head ----
  loss_ref, z_ref, _, head_grads, dlast = head_reference(nhwc(nl - 1, "post"), keep, vec, y, sd0)
  ledger.allclose("head", "z", tr.z, z_ref, rtol=1e-4, atol=2e-5)
  ledger.allclose("head", "loss", loss.reshape(1), loss_ref.reshape(1), rtol=2e-5, atol=0.0)
  for k in HEAD_KEYS:
    ledger.backward("head", k, grads[k], head_grads[k])
  ledger.backward("head", "dpost[%d]" % (nl - 1), nhwc(nl - 1, "grad"), dlast)
  del head_grads, dlast

  # ---- conv stack ----
  res_writer = {l.res_from: l.index for l in table if l.res_from >= 0}  # block input -> the projection that also writes its gradient
  for l in table:
    i = l.index
    W = sd0[l.conv + ".weight"]
    gamma, beta = sd0[l.bn + ".weight"], sd0[l.bn + ".bias"]
    rm0, rv0 = sd0[l.bn + ".running_mean"], sd0[l.bn + ".running_var"]
    x = nhwc(i - 1, "post") if i else visual.permute(0, 2, 3, 1)
    pre, post, dpost = nhwc(i, "pre"), nhwc(i, "post"), nhwc(i, "grad")
    ledger.forward("conv", l.conv, pre, R.conv_forward(l.kind, x, W, l.stride))
    residual = nhwc(l.res_from, "post") if l.res_from >= 0 else None
    post_ref, rm_ref, rv_ref = R.bn_act_forward(pre, gamma, beta, rm0, rv0, train, l.relu6, residual)
    ledger.forward("bn-act", l.bn, post, post_ref)
    del post_ref, residual
    if train:
      ledger.allclose("running", l.bn + ".running_mean", sd1[l.bn + ".running_mean"], rm_ref, rtol=1e-4, atol=2e-6)
      ledger.allclose("running", l.bn + ".running_var", sd1[l.bn + ".running_var"], rv_ref, rtol=1e-4, atol=2e-6)
    else:
      assert torch.equal(sd1[l.bn + ".running_mean"], rm0) and torch.equal(sd1[l.bn + ".running_var"], rv0), l.bn
    g = R.layer_backward(l.kind, x, W, l.stride, pre, post, dpost, gamma, rm0, rv0, train, l.relu6, need_dx=i > 0)
    ledger.backward("dbeta", l.bn + ".bias", grads[l.bn + ".bias"], g.dbeta, floor=1e-6 * g.dbeta_abs.max())
    ledger.backward("dgamma", l.bn + ".weight", grads[l.bn + ".weight"], g.dgamma, floor=1e-6 * g.dgamma_abs.max())
    ledger.backward("dW", l.conv + ".weight", grads[l.conv + ".weight"], g.dW)
    if i:
      want = g.dx
      if i - 1 in res_writer:  # the two writers `encoder_backward` documents
        want = want + nhwc(res_writer[i - 1], "grad").to(F64)
      ledger.backward("dx", "dpost[%d]" % (i - 1), nhwc(i - 1, "grad"), want)
      del want
    del g, x, pre, post, dpost  # the float64 temporaries of features.2's expansion are 0.53 GB each at B = 277

  # the running-statistic slots of the gradient vector hold zeros
  for l in table:
    assert not bool(grads[l.bn + ".running_mean"].any()) and not bool(grads[l.bn + ".running_var"].any())
  tag = "B=%d C=%d %s%s:" % (B, C, "train" if train else "frozen", " deterministic" if deterministic else "")
  worst = ledger.settle(tag, nonzero_families=("conv", "bn-act", "running", "dW", "dx", "head"))
  torch.cuda.synchronize()
  print("%s %d checks over %d layers and the head in %.2f s" % (tag, len(ledger.rows), nl, time.perf_counter() - t0))
  assert set(worst) == {"head", "conv", "bn-act", "dbeta", "dgamma", "dW", "dx"} | ({"running"} if train else set())
  assert sum(r[0] == "conv" for r in ledger.rows) == sum(r[0] == "dW" for r in ledger.rows) == 52
  assert sum(r[0] == "dx" for r in ledger.rows) == 51
  tr.close()
