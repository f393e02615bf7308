"""The CIL training step (oatomobile/baselines/torch/cil/train.py:168-219): `CILTrainer` / `rip_cil_train_*` against
the reference's own step (tests/golden/g16_cil_train_step.npz, tools/make_golden_host.py) and against a CPU
restatement of the step on `oracle.cil.OracleBehaviouralModel`, which is itself pinned to g16 here (no GPU needed)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oatomobile_amd import weights as W
from tests.helpers import synth_observation

CTX_KEYS = ("visual_features", "velocity", "is_at_traffic_light", "traffic_light_state", "mode")


# ---------------------------------------------------------------------------------------------------------
# CPU restatement of cil/train.py:168-190 (autograd on the oracle's BehaviouralModel)
# ---------------------------------------------------------------------------------------------------------
def trainable_cil(sd, T=4):
  """OracleBehaviouralModel with trainable parameters in train mode, the classifier's Dropout replaced by a caller-given
  mask and every ReLU6 of the encoder by one that can take the kink decisions of another implementation (as
  oracle.train_cpu.trainable_model does for the DIM model)."""
  from oracle import train_cpu as TC
  from oracle.cil import OracleBehaviouralModel
  m = OracleBehaviouralModel(output_shape=(T, 2))
  m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
  for p in m.parameters():
    p.requires_grad_(True)
  m._encoder._model.classifier[0] = TC._MaskedDropout()

  def swap(mod):
    for name, child in mod.named_children():
      if isinstance(child, torch.nn.ReLU6):
        setattr(mod, name, TC._KinkReLU6())
      else:
        swap(child)

  swap(m._encoder)
  m.train()
  return m


def cil_loss_and_grads(m, ctx, target, dropout_mask):
  """cil/train.py:174-183: predictions, L1 loss summed over [-2, -1] and averaged over the batch, backward.  Returns
  (loss, predictions); gradients are left in `p.grad`."""
  for p in m.parameters():
    p.grad = None
  m._encoder._model.classifier[0].mask = dropout_mask
  predictions = m(**ctx)
  loss = torch.nn.L1Loss(reduction="none")(predictions, target)
  loss = torch.mean(torch.sum(loss, dim=[-2, -1]), dim=0)
  loss.backward()
  return loss.detach(), predictions.detach()


def replay_reference_kinks(m, g, t, ctx, target, mask):
  """The oracle's own ReLU6 decisions, except at the elements g16 recorded within `kink_window` of a kink, which take
  the reference's (see tests/test_oracle_golden.py:replay_reference_kinks; a probe copy keeps the running statistics)."""
  from oracle import train_cpu as TC
  probe = copy.deepcopy(m)
  TC.set_kink_masks(probe, None)
  pre = []
  for mod in TC.kink_modules(probe):
    mod.register_forward_pre_hook(lambda mod, inp: pre.append(inp[0].detach().clone()))
  cil_loss_and_grads(probe, ctx, target, mask)
  post = []
  for i, x in enumerate(pre):
    p = x.clamp(0.0, 6.0).reshape(-1)
    idx = torch.from_numpy(g[t + "kink:%d:idx" % i].astype(np.int64))
    p[idx] = torch.from_numpy(g[t + "kink:%d:pass" % i]).to(p.dtype) * 3.0  # inside (0, 6): passes; 0: blocked
    post.append(p.view_as(x))
  TC.set_kink_masks(m, post)


def test_g16_cil_train_step_restatement_vs_reference(golden):
  """The CPU restatement against the reference's own BehaviouralModel run through cil/train.py:168-190 (two Adam steps
  with weight decay, train mode): loss, predictions, sampled gradients, post-step parameters, BatchNorm running
  statistics; the same tolerances as the g15 oracle test.  This pins the checker the GPU tests below use."""
  from tests.test_oracle_golden import check_train_tensors
  torch.set_num_threads(1)
  g = golden("g16_cil_train_step.npz")
  T = int(g["T"])
  m = trainable_cil(W.synthetic_cil_state_dict(int(g["weight_seed"])), T).double()
  opt = torch.optim.Adam(m.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
  params = dict(m.named_parameters())
  for step in range(2):
    t = "s%d_" % step
    ctx = {k: torch.from_numpy(g[t + k]).double() for k in CTX_KEYS}
    target = torch.from_numpy(g[t + "player_future"][..., :2]).double()
    mask = torch.from_numpy(g[t + "dropout_mask"]).double()
    replay_reference_kinks(m, g, t, ctx, target, mask)
    loss, pred = cil_loss_and_grads(m, ctx, target, mask)
    np.testing.assert_allclose(float(loss), float(g[t + "loss"]), rtol=1e-5)
    np.testing.assert_allclose(pred.numpy(), g[t + "predictions"], rtol=1e-4 if step == 0 else 1e-3,
                               atol=1e-5 if step == 0 else 1e-4)
    gn = float(torch.sqrt(sum((p.grad**2).sum() for p in m.parameters())))
    np.testing.assert_allclose(gn, float(g[t + "grad_norm"]), rtol=1e-3 if step == 0 else 2e-2)
    grads = {k: params[k].grad.detach().numpy().copy() for k in map(str, g["keys"])}
    opt.step()
    check_train_tensors(g, t, grads, {k: params[k].detach().numpy() for k in map(str, g["keys"])},
                        rtol=2e-3 if step == 0 else 3e-2, atol_frac=2e-4 if step == 0 else 2e-2)
    sd = m.state_dict()
    for key in g.files:
      if key.startswith(t + "buffer:"):
        name = key[len(t + "buffer:"):]
        if name.endswith("num_batches_tracked"):
          continue  # the restatement's model is rebuilt from a state_dict whose counters are the synthetic ones
        # (step 1: the statistics of a forward through parameters that carry step 0's rounding-decided Adam moves)
        np.testing.assert_allclose(sd[name].numpy(), g[key], rtol=1e-5 if step == 0 else 1e-4, atol=1e-6, err_msg=key)
    with torch.no_grad():  # step 1 starts from the reference's values of the noise-gradient coordinates
      for key in g.files:
        if key.startswith(t + "noise:") and key.endswith(":idx"):
          p = params[key[len(t + "noise:"):-len(":idx")]].view(-1)
          p[torch.from_numpy(g[key].astype(np.int64))] = torch.from_numpy(g[key[:-len(":idx")] + ":val"]).to(p.dtype)


def test_cil_train_numel_is_the_packed_spec():
  """rip_cil_train_numel == the BehaviouralModel state_dict minus its num_batches_tracked counters (host-only call)."""
  from oatomobile_amd import _lib, arch
  lib = _lib.load()
  for C in (2, 4):
    want = sum(int(np.prod(s)) for k, s in arch.cil_state_dict_spec(C) if not k.endswith("num_batches_tracked"))
    assert int(lib.rip_cil_train_numel(C)) == want
    # against DIM's layout: the merger's first layer is one column (`mode`) wider, _output replaces the flow's head
    assert want - int(lib.rip_train_numel(C)) == 64 + (2 * 64 + 2) - (32 * 64 + 32 + 4 * 32 + 4)
  assert int(lib.rip_cil_train_numel(0)) == 0


# ---------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _rel_l2(a, b):
  return float(np.sqrt(((a.astype(np.float64) - b)**2).sum() / max((b.astype(np.float64)**2).sum(), 1e-30)))


def hip_cil(seed, T, dev):
  from oatomobile_amd import BehaviouralModel
  return BehaviouralModel.synthetic(seed, output_shape=(T, 2)).to(dev)


def make_batch(rng, B, T, dev):
  """B synthetic observations as `transform` leaves them, device and CPU copies (mode in {0, 2, 3})."""
  from oatomobile_amd import transform_visual
  obs = [synth_observation(rng) for _ in range(B)]
  lid = torch.stack([torch.from_numpy(o["lidar"]) for o in obs]).to(dev)
  ctx = dict(visual_features=transform_visual(lid, channels_last=True),
             velocity=torch.stack([torch.from_numpy(o["velocity"]) for o in obs]).to(dev),
             is_at_traffic_light=torch.tensor([[float(o["is_at_traffic_light"])] for o in obs], device=dev),
             traffic_light_state=torch.tensor([[float(o["traffic_light_state"])] for o in obs], device=dev),
             mode=torch.from_numpy(rng.choice([0.0, 2.0, 3.0], size=(B, 1)).astype(np.float32)).to(dev))
  return ctx, {k: v.cpu() for k, v in ctx.items()}


@pytest.mark.gpu
def test_g16_cil_train_step_vs_reference(golden, dev):
  """Two consecutive CILTrainer steps (train mode, dropout mask replayed, Adam with weight decay) against the
  reference's own BehaviouralModel run through train_step.  Held tightly: loss, predictions, BatchNorm running
  statistics, the gradient norm; per element the gradients of the decoder, output layer, merger and classifier (no
  ReLU6 between them and the loss) and their post-Adam parameters; the encoder's gradients, defined up to the ReLU6
  kink decisions, in relative L2 (the per-element check is test_cil_backward_vs_restatement_same_kinks)."""
  from oatomobile_amd import CILTrainer
  g = golden("g16_cil_train_step.npz")
  T = int(g["T"])
  tr = CILTrainer(hip_cil(int(g["weight_seed"]), T, dev), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]),
                  max_batch=8, device=dev)
  for step in range(2):
    t = "s%d_" % step
    batch = {k: torch.from_numpy(g[t + k]).to(dev) for k in CTX_KEYS + ("player_future",)}
    loss = tr.backward(batch, dropout_mask=torch.from_numpy(g[t + "dropout_mask"]))
    print("g16 step %d: loss %.6f (reference %.6f)" % (step, float(loss), float(g[t + "loss"])))
    np.testing.assert_allclose(float(loss), float(g[t + "loss"]), rtol=2e-5 if step == 0 else 2e-3)
    np.testing.assert_allclose(tr.predictions.cpu().numpy(), g[t + "predictions"], rtol=1e-4 if step == 0 else 5e-2,
                               atol=2e-5 if step == 0 else 5e-2)
    grads = {k: v.cpu().numpy().copy() for k, v in tr.named_gradients().items()}
    gn = float(torch.linalg.vector_norm(tr.grads.double()))
    np.testing.assert_allclose(gn, float(g[t + "grad_norm"]), rtol=5e-3 if step == 0 else 0.15)
    tr.apply()
    params = {k: v.cpu().numpy() for k, v in tr.state_dict().items()}
    worst = 0.0
    for k in map(str, g["keys"]):
      smooth = not k.startswith("_encoder._model.features")  # classifier, merger, GRU, output: no ReLU6 to the loss
      if t + "grad:" + k in g.files:
        gref, gact = g[t + "grad:" + k].reshape(-1), grads[k].reshape(-1)
        pref, pact = g[t + "param:" + k].reshape(-1), params[k].reshape(-1)
      else:
        idx = g[t + "grad:" + k + ":idx"]
        gref, gact = g[t + "grad:" + k + ":val"], grads[k].reshape(-1)[idx]
        pref, pact = g[t + "param:" + k + ":val"], params[k].reshape(-1)[idx]
      if np.abs(gref).max() < 1e-6:
        continue
      err = _rel_l2(gact, gref)
      worst = max(worst, err)
      if smooth and step == 0:
        np.testing.assert_allclose(gact, gref, rtol=1e-3, atol=1e-6 + 1e-4 * np.abs(gref).max(), err_msg=k)
        solid = np.abs(gref) > 1e-5 + 1e-3 * np.abs(gref).max()
        np.testing.assert_allclose(pact[solid], pref[solid], rtol=1e-4, atol=2e-5, err_msg="param:" + k)
      elif step == 0:
        assert err < 0.02, (k, err)
    print("g16 step %d: worst relative L2 gradient deviation over %d recorded tensors: %.3g" % (step, len(g["keys"]), worst))
    for key in g.files:
      if key.startswith(t + "buffer:"):
        name = key[len(t + "buffer:"):]
        if name.endswith("num_batches_tracked"):
          assert int(params[name]) == int(g[key])
        else:
          np.testing.assert_allclose(params[name], g[key], rtol=1e-4 if step == 0 else 2e-2,
                                     atol=2e-6 if step == 0 else 1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [4, 40])
@pytest.mark.parametrize("train", [True, False])
def test_cil_backward_vs_restatement_same_kinks(dev, T, train):
  """Every gradient tensor per element against the CPU restatement differentiating the same piecewise-linear function:
  the restatement takes the ReLU6 kink decisions of the HIP forward (rip_train_peek), and the targets keep every
  |prediction - target| at least 0.5 from the L1 kink (asserted on the HIP predictions).  T = 4 (the reference's
  training horizon) and T = 40 (CILAgent's), batch-statistics (dropout mask given) and eval-mode BatchNorm (no
  dropout)."""
  from oatomobile_amd import CILTrainer, arch
  from oracle import train_cpu as TC
  B = 9
  sd = W.synthetic_cil_state_dict(33)
  mo = trainable_cil(sd, T)
  if not train:
    mo.eval()
  tr = CILTrainer(hip_cil(33, T, dev), lr=1e-3, max_batch=16, device=dev)
  rng = np.random.default_rng(330 + T)
  ctx, cpu = make_batch(rng, B, T, dev)
  mask = torch.from_numpy(((rng.random((B, 1280)) >= 0.2) / 0.8).astype(np.float32)) if train else None
  probe = copy.deepcopy(mo)  # (a train-mode forward updates the running statistics)
  with torch.no_grad():
    probe._encoder._model.classifier[0].mask = mask
    p0 = probe(**cpu)
  off = torch.from_numpy((rng.choice([-1.0, 1.0], size=(B, T, 2)) * rng.uniform(0.6, 1.5, size=(B, T, 2))).astype(np.float32))
  target = p0 + off
  loss = tr.backward(dict(ctx, player_future=target.to(dev)), dropout_mask=mask, train=train)
  pred = tr.predictions.cpu()
  margin = float((pred - target).abs().min())
  assert margin > 0.5, margin
  posts = [tr.peek(i, "post").cpu() for i, l in enumerate(arch.conv_layers(2)) if l.relu6]
  captured = []
  hooks = [mod.register_forward_hook(lambda md, inp, out: captured.append(out.detach())) for mod in TC.kink_modules(mo)]
  loss_o, pred_o = cil_loss_and_grads(mo, cpu, target, mask)
  for hk in hooks:
    hk.remove()
  flips = sum(int((((a > 0) & (a < 6)) != ((b > 0) & (b < 6))).sum()) for a, b in zip(posts, captured))
  fwd = max(float((a - b).abs().max()) for a, b in zip(posts, captured))
  print("T=%d train=%s: %d of %d ReLU6 decisions differ between the HIP and the CPU forward (max |d activation| %.2g), "
        "min |pred - target| %.3f" % (T, train, flips, sum(a.numel() for a in posts), fwd, margin))
  assert flips < 100 and fwd < 1e-3
  np.testing.assert_allclose(float(loss), float(loss_o), rtol=2e-5)
  # held against the plan scale (as test_gpu_parity.py's g10 test holds CILAgent): a 40-step roll-out amplifies a z
  # difference — here the ~1e-4 of the ReLU6 decisions the two forwards take differently — roughly a thousandfold by
  # its last step in train mode (the restatement's own fp32 and fp64 runs of this batch: 3e-7 at t = 0, 3.5e-4 at
  # t = 39, max |pred| 11.7; HIP against the fp32 restatement measured 1.3e-3)
  np.testing.assert_allclose(pred.numpy(), pred_o.numpy(), rtol=1e-4, atol=2e-4 * max(1.0, float(pred_o.abs().max())))
  if train:
    mo.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})  # undo the running-stat update
  TC.set_kink_masks(mo, posts)
  cil_loss_and_grads(mo, cpu, target, mask)
  hg = tr.named_gradients()
  worst = 0.0
  gmax = max(float(p.grad.abs().max()) for p in mo.parameters())
  # the train-mode 40-step roll-out is the ill-conditioned case (see the predictions above): there the restatement's own
  # fp32 and fp64 gradients differ by 2.8e-4 of each tensor's scale (1e-5 at T = 4 and in eval mode), and HIP against
  # the fp32 restatement measured 8.7e-4 and 1.2e-3 in two runs (the encoder's split-K atomics vary run to run)
  frac = 3e-3 if (T == 40 and train) else 3e-4
  for k, p in mo.named_parameters():
    go, gh = p.grad.numpy(), hg[k].cpu().numpy()
    scale = np.abs(go).max()
    if scale < 1e-6 * gmax:
      continue  # mathematically zero (a BN bias in front of another batch-statistics BN): rounding noise on both sides
    worst = max(worst, np.abs(gh - go).max() / scale)
    np.testing.assert_allclose(gh, go, rtol=2e-3, atol=1e-6 + frac * scale, err_msg=k)
  print("T=%d train=%s: worst max|dgrad| / max|grad| over the parameter tensors with the same kinks: %.3g" % (T, train, worst))


@pytest.mark.gpu
def test_cil_evaluate_step_is_inference_and_agent_hand_back(dev):
  """A few Adam steps; then evaluate_step (cil/train.py:208-219) predicts what BehaviouralModel.forward predicts from
  the same weights (1e-4) and its loss is the restatement's in eval mode; after sync_to_model, CILAgent (T = 40) plans
  what oracle.cil.cil_call plans with the trained state_dict."""
  from oatomobile_amd import CILAgent, CILTrainer
  from oracle import cil as C
  T, B = 40, 6
  m = hip_cil(37, T, dev)
  tr = CILTrainer(m, lr=1e-3, weight_decay=1e-4, max_batch=8, device=dev)
  nbt0 = tr.num_batches_tracked
  rng = np.random.default_rng(370)
  ctx, cpu = make_batch(rng, B, T, dev)
  future = torch.from_numpy(np.cumsum(np.abs(rng.normal(size=(B, T, 3))) * 0.5, axis=1).astype(np.float32))
  batch = dict(ctx, player_future=future.to(dev))
  losses = [float(tr.train_step(batch)) for _ in range(3)]
  assert tr.step_count == 3 and tr.num_batches_tracked == nbt0 + 3 and all(np.isfinite(losses))
  ev = float(tr.evaluate_step(batch))
  pred_ev = tr.predictions.cpu().numpy()
  trained = {k: v.cpu().numpy() for k, v in tr.state_dict().items()}
  tr.sync_to_model()
  with torch.no_grad():
    pred_inf = m(**ctx).cpu().numpy()
  print("evaluate_step vs BehaviouralModel.forward: max|d pred| %.3g" % np.abs(pred_ev - pred_inf).max())
  np.testing.assert_allclose(pred_ev, pred_inf, rtol=1e-4, atol=1e-4)
  mo = C.OracleBehaviouralModel.from_numpy_state_dict(trained)  # eval mode, T = 40
  with torch.no_grad():
    pred_o = mo(**cpu)
  ev_o = float(torch.abs(pred_o - future[..., :2]).sum(dim=[-2, -1]).mean())
  print("evaluate_step loss %.5f (restatement on the same weights %.5f)" % (ev, ev_o))
  np.testing.assert_allclose(ev, ev_o, rtol=1e-4)
  np.testing.assert_allclose(pred_ev, pred_o.numpy(), rtol=1e-4, atol=1e-4)
  agent = CILAgent(None, model=m, device=dev)
  for i, goal_last in enumerate([(1.0, 0.5), (10.0, 12.0), (20.0, 1.0)]):  # STOP, LEFT, RIGHT
    ob = synth_observation(np.random.default_rng(371 + i))
    ob["goal"] = np.asarray(ob["goal"], np.float32).copy()
    ob["goal"][-1, :2] = goal_last
    plan = agent(dict(ob))
    ref = C.cil_call(mo, ob)
    np.testing.assert_allclose(plan, ref, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(ref).max()))


@pytest.mark.gpu
def test_cil_forward_outputs_repeat(dev):
  """Two identical forward calls give the same loss and predictions.  (Bit-identity is not a property of this step:
  the encoder's deep pointwise convolutions run as split-K GEMMs that add their K chunks with float atomics — see
  test_gpu_parity.py:test_train_batch_statistics_are_the_same_bits_on_every_run — so z, and what the decoder makes of
  it, may move in the last place.  The decoder kernel itself is deterministic: lanes reduce in a fixed order.)"""
  from oatomobile_amd import CILTrainer
  T, B = 4, 5
  tr = CILTrainer(hip_cil(38, T, dev), max_batch=8, device=dev)
  rng = np.random.default_rng(380)
  ctx, _ = make_batch(rng, B, T, dev)
  batch = dict(ctx, player_future=torch.from_numpy(rng.normal(size=(B, T, 2)).astype(np.float32)).to(dev))
  outs = []
  for _ in range(2):
    loss = tr.evaluate_step(batch)
    outs.append((loss.cpu().numpy(), tr.predictions.cpu().numpy()))
  (l0, p0), (l1, p1) = outs
  print("repeat: loss bits equal %s, predictions bits equal %s" % (l0.tobytes() == l1.tobytes(), p0.tobytes() == p1.tobytes()))
  np.testing.assert_allclose(l0, l1, rtol=1e-6)
  np.testing.assert_allclose(p0, p1, rtol=1e-6, atol=1e-6)


@pytest.mark.gpu
def test_cil_trainer_errors(dev):
  """The error paths DIMTrainer has: CPU tensors, B > max_batch, wrong shapes; a missing `mode`; a DIM handle given to
  the CIL entry point and a CIL handle to the DIM one (RIP_EINVAL, nothing launched)."""
  from oatomobile_amd import CILTrainer, DIMTrainer, ImitativeModel, _lib
  T = 4
  tr = CILTrainer(hip_cil(39, T, dev), max_batch=4, device=dev)
  rng = np.random.default_rng(390)
  ctx, cpu = make_batch(rng, 5, T, dev)
  target = torch.zeros(5, T, 2, device=dev)
  small = {k: v[:3] for k, v in ctx.items()}
  with pytest.raises(RuntimeError, match="no CPU path"):
    tr.backward(dict({k: v[:3] for k, v in cpu.items()}, player_future=target[:3].cpu()))
  with pytest.raises(ValueError, match="max_batch"):
    tr.backward(dict(ctx, player_future=target))
  with pytest.raises(ValueError, match="mode"):
    tr.backward(dict({k: v for k, v in small.items() if k != "mode"}, player_future=target[:3]))
  with pytest.raises(ValueError):
    tr.backward(dict(small, player_future=torch.zeros(3, T + 1, 2, device=dev)))
  with pytest.raises(ValueError):
    tr.backward(dict(small, visual_features=small["visual_features"][:, :1].contiguous(), player_future=target[:3]))
  dim = DIMTrainer(ImitativeModel.synthetic(39).to(dev), max_batch=4, device=dev)
  lib = _lib.load()
  vis = small["visual_features"].contiguous()
  vec6 = torch.zeros(3, 6, device=dev)
  loss = torch.zeros(1, device=dev)
  stream = _lib.current_stream(dev)
  rc = lib.rip_cil_train_forward_backward(dim._h, _lib.ptr(dim.params), None, _lib.ptr(vis), _lib.ptr(vec6),
                                          _lib.ptr(target), None, 3, 1, _lib.ptr(loss), None, stream)
  assert rc != 0
  rc = lib.rip_train_forward_backward(tr._h, _lib.ptr(tr.params), None, _lib.ptr(vis), _lib.ptr(vec6[:, :5].contiguous()),
                                      _lib.ptr(target), None, 3, 1, _lib.ptr(loss), None, stream)
  assert rc != 0
  torch.cuda.synchronize(dev)
  # both trainers still work after the refused calls
  assert np.isfinite(float(tr.evaluate_step(dict(small, player_future=target[:3]))))
  tr.close()
  dim.close()
  with pytest.raises(ValueError, match="visual_features"):
    CILTrainer(hip_cil(39, T, dev), max_batch=4, device=dev).backward({})


@pytest.mark.gpu
def test_cil_overfits_one_batch(dev):
  """200 Adam steps (lr 1e-2) on one fixed batch of 16 with targets of about 1 m: the last train-mode loss is at most
  half the first.  Catches sign and transposition errors that a single step can hide.  The CPU restatement over the
  same 200 steps (same batch and weights, its own dropout draws) went from 3.910 to 0.386, a ratio of 0.099; the
  threshold 0.5 leaves the room that different dropout draws need."""
  from oatomobile_amd import CILTrainer
  T, B = 4, 16
  tr = CILTrainer(hip_cil(36, T, dev), lr=1e-2, max_batch=B, device=dev)
  rng = np.random.default_rng(360)
  ctx, _ = make_batch(rng, B, T, dev)
  target = torch.from_numpy(np.cumsum(np.abs(rng.normal(size=(B, T, 2))) * 0.25, axis=1).astype(np.float32))
  batch = dict(ctx, player_future=target.to(dev))
  torch.manual_seed(0)
  losses = [float(tr.train_step(batch)) for _ in range(200)]
  print("overfit: first %.4f, last %.4f, ratio %.3f" % (losses[0], losses[-1], losses[-1] / losses[0]))
  assert np.isfinite(losses).all()
  assert losses[-1] <= 0.5 * losses[0]
