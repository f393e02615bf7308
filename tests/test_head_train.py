"""The K-member head step on cached encoder features: `rip_head_forward_backward` (csrc/head_train.hip) through
`train.HeadTrainer`, `RIPAgent.features_batch` and `replay.FeatureCache`, against the float64 restatement of
tests/head_ref.py and against the shipped inference kernels.

Metric of the parity tests: max|d - d_ref| / max(1, max|d_ref|) <= 1e-4 (`TOL` of tests/test_flow_autograd.py) for
q_rows, loss, z and every gradient tensor of every member.  Worst values measured on the MI355X over the six synthetic
cases and the real-feature case (`pytest -s` prints each): q_rows 2.2e-7, loss 2.2e-7, z 4.1e-7, gradients 4.6e-6
(`_decoder._decoder.weight_ih` at the far-off row, whose y_prev of 100 - 150 m multiplies the gate gradients; every other
tensor at most 8.7e-7).  `evaluate_step` against `score_trajectories`: 0 (the same values).  Learning curve: largest
relative deviation from the float64 curve 1.52e-7 (bound 1.6e-6)."""

import numpy as np
import pytest
import torch

from tests import head_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4
WORST = {}
MAX_BATCH = 128


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  torch.cuda.set_device(0)
  return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def agents(dev):
  """K -> a RIPAgent over the K synthetic members of head_ref.MEMBER_SEEDS (max_batch 8)."""
  from oatomobile_amd import ImitativeModel, RIPAgent
  cache = {}

  def get(K):
    if K not in cache:
      models = [ImitativeModel.synthetic(s) for s in R.MEMBER_SEEDS[:K]]
      cache[K] = RIPAgent(None, algorithm="WCM", models=models, num_candidates=16, max_batch=8, device=dev)
    return cache[K]

  return get


def trainer_for(agent, heads=None, **kw):
  from oatomobile_amd.train import HeadTrainer
  kw.setdefault("max_batch", MAX_BATCH)
  tr = HeadTrainer(agent, **kw)
  if heads is not None:
    tr.params.copy_(torch.as_tensor(heads, device=tr.params.device))
  return tr


def t(a, dev, dtype=torch.float32):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev).contiguous()


def _check(tag, key, got, want):
  got = got.detach().cpu().numpy().astype(np.float64)
  want = np.asarray(want, np.float64)
  assert got.shape == want.shape, (tag, key, got.shape, want.shape)
  err = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
  WORST[key] = max(WORST.get(key, 0.0), err)
  print("%s %s: %.3g" % (tag, key, err))
  assert err <= TOL, "%s %s: max|d - d_ref| / max(1, max|d_ref|) = %.3g" % (tag, key, err)


def _parity(tag, tr, heads, feat, vec, y, dev):
  """One backward of `tr` on (feat [K,B,128], vec [B,5], y [K,B,4,2]) against head_ref in float64, then forward only."""
  K = heads.shape[0]
  loss = tr.backward(t(feat, dev), t(vec, dev), y=t(y, dev))
  q_train = tr.q_rows.clone()
  for k in range(K):
    ref = R.head_ref(R.head_model(heads[k]), feat[k], vec, y[k])
    assert ref["min_pre"] >= R.KINK_MARGIN, (tag, k, ref["min_pre"])
    _check(tag, "q_rows", tr.q_rows[k], ref["q_rows"])
    _check(tag, "loss", loss[k], ref["loss"])
    _check(tag, "z", tr.z[k], ref["z"])
    named = tr.named_gradients(k)
    assert list(named) == R.HEAD_KEYS
    for key in R.HEAD_KEYS:
      _check(tag + " " + key, "grads", named[key], ref["grads"][key])
  q_eval = tr.evaluate_step(t(feat, dev), t(vec, dev), y=t(y, dev))
  assert torch.equal(q_eval, q_train), "%s: forward-only q_rows differ from the training mode's" % tag
  return loss


@pytest.mark.parametrize("K, B", sorted(R.CASE_SEEDS))
def test_parity_with_float64(dev, agents, K, B):
  """K in {1, 3} x B in {1, 5, 67}: one row, fewer rows than waves in a workgroup, a grid-stride remainder with 4B not
  a multiple of the weight-gradient tile; distinct weights per member, a far-off target row, and in (3, 5) a merger
  unit that is dead on every row."""
  case = R.make_case(K, B)
  tr = trainer_for(agents(K), case["heads"])
  _parity("K=%d B=%d" % (K, B), tr, case["heads"], case["feat"], case["vec"], case["y"], dev)
  if (K, B) == (3, 5):
    g = tr.named_gradients(0)
    assert float(g["_merger._model.0.weight"][R.DEAD_UNIT].abs().max()) == 0.0 and float(g["_merger._model.0.bias"][R.DEAD_UNIT]) == 0.0


def test_parity_on_real_features(dev, agents):
  """Features from `RIPAgent.features_batch` on random 200 x 200 x 2 BEVs; its z (the inference merger kernel) agrees
  with the training kernel's."""
  case = R.real_case_inputs()
  agent = agents(R.REAL_K)
  feat, z = agent.features_batch(t(case["lidar"], dev), t(case["vec"], dev))
  assert feat.shape == (R.REAL_K, R.REAL_B, 128) and z.shape == (R.REAL_K, R.REAL_B, 64)
  tr = trainer_for(agent)
  assert torch.equal(tr.params.cpu(), torch.as_tensor(case["heads"]))
  _parity("real", tr, case["heads"], feat.cpu().numpy(), case["vec"], case["y"], dev)
  _check("real", "z", tr.z, z.cpu().numpy())


def _snapshot(tr, loss):
  return dict(loss=loss.clone(), q=tr.q_rows.clone(), z=tr.z.clone(), g=tr.grads.clone())


def _assert_same_bits(a, b, what, members=None):
  for key in a:
    x, y = (a[key], b[key]) if members is None else (a[key][members], b[key][members])
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "%s: %s differs" % (what, key)


def test_row_indirection(dev, agents):
  """`rows` with repeats and a reversed order, `future` with L = 8 and stride 2 plus noise: bit-equal to the same call on
  explicitly gathered dense inputs; an out-of-range row gives NaN for its member alone."""
  K, n, B, L = 3, 11, 7, 8
  rng = np.random.default_rng(31)
  agent = agents(K)
  heads = R.case_heads(K)
  feat = t(R.FEAT_SCALE * rng.standard_normal((K, n, 128)), dev)
  vec = t(R.case_vec(rng, n), dev)
  future = t(np.cumsum(np.abs(rng.normal(size=(n, L, 2))) * 0.8, axis=1), dev)
  noise = t(0.01 * rng.standard_normal((K, B, 4, 2)), dev)
  shared = torch.tensor([10, 9, 9, 3, 0, 3, 10], device=dev)
  tr = trainer_for(agent, heads)
  # the same rows for every member: ONE dense K = 3 call is the reference
  rows = shared.unsqueeze(0).expand(K, -1).contiguous()
  got = _snapshot(tr, tr.backward(feat, vec, target=future, rows=rows, noise=noise))
  dense_y = future[shared][:, 0::2].unsqueeze(0) + noise
  want = _snapshot(tr, tr.backward(feat[:, shared].contiguous(), vec[shared].contiguous(), y=dense_y.contiguous()))
  _assert_same_bits(got, want, "shared rows")
  # rows of its own per member: member k against a K = 1 call on its gathered rows
  rows = torch.stack([shared, shared.flip(0), torch.tensor([0, 1, 2, 2, 2, 5, 6], device=dev)])
  got = _snapshot(tr, tr.backward(feat, vec, target=future, rows=rows, noise=noise))
  for k in range(K):
    one = trainer_for(agents(1), heads[k:k + 1])
    yk = (future[rows[k]][:, 0::2] + noise[k]).unsqueeze(0).contiguous()
    want = _snapshot(one, one.backward(feat[k:k + 1, rows[k]].contiguous(), vec[rows[k]].contiguous(), y=yk))
    _assert_same_bits({key: v[k:k + 1] for key, v in got.items()}, want, "member %d rows" % k)
  # a row outside [0, n): NaN for member 1 only
  bad = rows.clone()
  bad[1, 2] = n
  out = _snapshot(tr, tr.backward(feat, vec, target=future, rows=bad, noise=noise))
  assert torch.isnan(out["loss"][1]) and torch.isnan(out["q"][1, 2]) and torch.isnan(out["g"][1]).all()
  assert torch.isnan(out["z"][1, 2]).all() and not torch.isnan(out["q"][1, :2]).any()
  _assert_same_bits(out, got, "members beside the bad row", members=[0, 2])


def test_determinism_and_member_independence(dev, agents):
  """Two runs give the same bits; member k of a K = 3 launch equals a K = 1 launch of that member at the same B; so do the
  parameters and the Adam moments after three steps."""
  K, B = 3, 67
  case = R.make_case(K, B)
  feat, vec, y = t(case["feat"], dev), t(case["vec"], dev), t(case["y"], dev)
  tr = trainer_for(agents(K), case["heads"])
  first = _snapshot(tr, tr.backward(feat, vec, y=y))
  tr.grads.fill_(7.0)
  second = _snapshot(tr, tr.backward(feat, vec, y=y))
  _assert_same_bits(first, second, "two runs")
  ones = [trainer_for(agents(1), case["heads"][k:k + 1]) for k in range(K)]
  for k, one in enumerate(ones):
    alone = _snapshot(one, one.backward(feat[k:k + 1].contiguous(), vec, y=y[k:k + 1].contiguous()))
    _assert_same_bits({key: v[k:k + 1] for key, v in first.items()}, alone, "member %d alone" % k)
  for _ in range(3):
    tr.train_step(feat, vec, y=y)
    for k, one in enumerate(ones):
      one.train_step(feat[k:k + 1].contiguous(), vec, y=y[k:k + 1].contiguous())
  for k, one in enumerate(ones):
    for name in ("params", "exp_avg", "exp_avg_sq"):
      assert torch.equal(getattr(tr, name)[k:k + 1], getattr(one, name)), (k, name)
  assert tr.step_count == 3 and not torch.equal(tr.params.cpu(), torch.as_tensor(case["heads"]))


def test_adam_closed_form(dev, agents):
  """`apply` at step_count 1 and 2 against torch.optim.Adam's update in float64 on the trainer's own gradients (with
  weight decay): rtol 1e-6.  An element whose update nearly cancels it (|p| ~ lr) carries the fp32 rounding of the
  subtraction, and at step 2 the update lr * m / (sqrt(v) + eps) carries the few-eps32 rounding of its fp32 moments: about
  1e-3 * 3e-7 in absolute terms, which no relative bound on a tiny result covers: atol = 1e-6 * lr.  The moments' own
  bits are covered by the member-independence test."""
  K, B = 3, 5
  lr, wd, b1, b2, eps = (float(np.float32(x)) for x in (1e-3, 1e-2, 0.9, 0.999, 1e-8))  # the C ABI takes them as float32
  case = R.make_case(K, B)
  tr = trainer_for(agents(K), case["heads"], lr=lr, weight_decay=wd)
  feat, vec, y = t(case["feat"], dev), t(case["vec"], dev), t(case["y"], dev)
  p = tr.params.double().cpu().numpy()
  m, v = np.zeros_like(p), np.zeros_like(p)
  for step in (1, 2):
    tr.backward(feat, vec, y=y)
    g = tr.grads.double().cpu().numpy() + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr / (1 - b1**step) * m / (np.sqrt(v) / np.sqrt(1 - b2**step) + eps)
    tr.apply()
    assert tr.step_count == step
    np.testing.assert_allclose(tr.params.cpu().numpy(), p, rtol=1e-6, atol=1e-6 * lr)
    p = tr.params.double().cpu().numpy()  # the next step starts from the trainer's own fp32 state
    m, v = tr.exp_avg.double().cpu().numpy(), tr.exp_avg_sq.double().cpu().numpy()


def test_learning(dev, agents):
  """64 rows, K = 2, 40 steps under fixed noise: every member's loss ends below its start and the curve stays within ten
  times the margin tests/test_head_train_cpu.py measures (fp32 against float64 of head_ref) of head_ref's float64 curve."""
  case = R.learning_case()
  tr = trainer_for(agents(R.LEARN_K), case["heads"], lr=R.LEARN_LR)
  feat, vec, target, noise = (t(case[key], dev) for key in ("feat", "vec", "target", "noise"))
  losses = torch.stack([tr.train_step(feat, vec, target=target, noise=noise[s]) for s in range(R.LEARN_STEPS)]).cpu().numpy()
  ref = R.learning_curve(case, torch.float64)
  dev_rel = float(np.max(np.abs(losses - ref) / np.abs(ref)))
  print("learning: losses %s -> %s, largest relative deviation from float64 %.3g" % (losses[0], losses[-1], dev_rel))
  assert np.all(losses[-1] < losses[0])
  assert dev_rel <= 10 * R.LEARNING_MARGIN


# ---------------------------------------------------------------------------------------------------------------------
# against the shipped inference kernels
# ---------------------------------------------------------------------------------------------------------------------
def _observations(dev, n, seed):
  from tests.helpers import synth_observation
  rng = np.random.default_rng(seed)
  obs = [synth_observation(rng, G=3) for _ in range(n)]
  lidar = t(np.stack([o["lidar"] for o in obs]), dev)
  vec = t(np.array([[*o["velocity"], o["is_at_traffic_light"], o["traffic_light_state"]] for o in obs]), dev)
  goal = t(np.stack([o["goal"][:, :2] for o in obs]), dev)
  y = t(R.case_targets(rng, 1, n)[0] * np.float32(0.5), dev)
  y[n - 1] = y[0] + 0.25  # (case_targets' far-off row is for the float64 parity; plan scale here)
  return lidar, vec, goal, y


def test_against_the_inference_kernels_and_publish(dev):
  from oatomobile_amd import ImitativeModel, RIPAgent, _lib, weights
  K, B, N = 2, 8, 16
  models = [ImitativeModel.synthetic(s) for s in (311, 312)]
  agent = RIPAgent(None, algorithm="WCM", models=models, num_candidates=N, max_batch=B, device=dev)
  lidar, vec, goal, y = _observations(dev, B, 88)
  tr = trainer_for(agent, max_batch=B)
  yk = y.unsqueeze(0).expand(K, -1, -1, -1).contiguous()

  def compare(tag):
    feat, z = agent.features_batch(lidar, vec)
    q = tr.evaluate_step(feat, vec, y=yk)
    want = agent.score_trajectories(lidar, vec, y).q
    _check(tag, "q_vs_inference", q, want.cpu().numpy())
    return feat

  feat = compare("before training")
  before = tr.params.clone()
  for _ in range(2):
    tr.train_step(feat, vec, y=yk)
  assert not torch.equal(before, tr.params)
  tr.publish(agent)
  assert torch.equal(compare("after publish"), feat)  # the encoders did not change
  for k in range(K):
    sd = {key: v.cpu().numpy() for key, v in tr.state_dict(k).items()}
    fresh = _lib.Handle(K, 2, B, 0, max_candidates=N)
    fresh.load_model(k, weights.pack_state_dict(sd))
    for which in range(8):
      assert torch.equal(agent._handle.peek_weights(k, which), fresh.peek_weights(k, which)), (k, which)
    a, b = agent._handle.model_flags(k), fresh.model_flags(k)
    assert np.float32(a[0]).view(np.uint32) == np.float32(b[0]).view(np.uint32) and a[1] == b[1]
  twins = [ImitativeModel.synthetic(s) for s in (311, 312)]
  for k, m in enumerate(twins):
    m.load_state_dict(tr.state_dict(k))
  other = RIPAgent(None, algorithm="WCM", models=twins, num_candidates=N, max_batch=B, device=dev)
  assert torch.equal(agent.plan_batch(lidar, vec, goal), other.plan_batch(lidar, vec, goal))
  tr.sync_to_models()
  for k in range(K):
    assert np.array_equal(models[k].packed_weights(), tr.full[k].cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# FeatureCache and train_epoch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coded_cache(dev):
  from oatomobile_amd import replay
  n, L = 11, 8
  rng = np.random.default_rng(17)
  codes = (rng.integers(0, 6, size=(n, 200, 200, 2)) * (rng.random((n, 200, 200, 2)) < 0.12)).astype(np.uint8)
  lut = np.zeros(256, np.float32)
  lut[:6] = np.arange(6, dtype=np.float32) / 5.0
  future = np.cumsum(np.abs(rng.normal(size=(n, L, 2))) * 0.8, axis=1)
  return replay.DeviceCache.from_tensors(t(codes, dev, torch.uint8), t(lut, dev), t(R.case_vec(rng, n), dev), t(future, dev),
                                         torch.zeros(n, device=dev))


def test_feature_cache(dev, coded_cache):
  from oatomobile_amd import ImitativeModel, RIPAgent, replay, weights
  data, bs = coded_cache, 4
  agent = RIPAgent(None, algorithm="WCM", models=[ImitativeModel.synthetic(s) for s in (411, 412)], max_batch=8, device=dev)
  cache = replay.FeatureCache.build(agent, data, bs)
  assert cache.feat.shape == (2, len(data), 128) and cache.vec is data.vec and cache.future is data.future
  for i0 in range(0, len(data), bs):
    feat, _ = agent.features_batch_coded(data.codes[i0:i0 + bs], data.lut, data.vec[i0:i0 + bs])
    assert torch.equal(cache.feat[:, i0:i0 + bs], feat), i0
  # the coded path's image is the float path's: features_batch on the decoded BEV gives the same bits
  decoded = data.lut[data.codes[:bs].long()]
  assert torch.equal(agent.features_batch(decoded, data.vec[:bs].contiguous())[0], cache.feat[:, :bs])
  assert cache.verify(agent)
  changed = torch.as_tensor(weights.pack_state_dict(weights.synthetic_state_dict(499)), device=dev)
  agent.load_member(1, changed)  # another encoder in member 1
  assert not cache.verify(agent)


@pytest.mark.parametrize("bootstrap", [False, True])
def test_train_epoch_draw_order(dev, coded_cache, agents, bootstrap):
  """`train_epoch` consumes the generator as documented (one randperm, then per batch the noise [K,rows,4,2]), trains the
  last short batch, and two identically seeded epochs give equal bits: a hand-written loop over `train_step` with the
  same draws reproduces it."""
  from oatomobile_amd import replay
  K, bs, n = 2, 4, len(coded_cache)
  rng = np.random.default_rng(23)
  cache = replay.FeatureCache(t(R.FEAT_SCALE * rng.standard_normal((K, n, 128)), dev), coded_cache.vec, coded_cache.future, bs,
                              coded_cache)
  member_rows = t(rng.integers(0, n, size=(K, 9)), dev, torch.int64) if bootstrap else None
  m = 9 if bootstrap else n
  heads = R.case_heads(K)
  runs = []
  for _ in range(2):
    tr = trainer_for(agents(K), heads)
    g = torch.Generator(device=dev).manual_seed(5)
    losses = tr.train_epoch(cache, bs, generator=g, member_rows=member_rows)
    assert losses.shape == (K,) and tr.step_count == (m + bs - 1) // bs == tr.last_epoch_losses.shape[0]
    runs.append((tr, g))
  assert torch.equal(runs[0][0].params, runs[1][0].params)
  hand = trainer_for(agents(K), heads)
  g = torch.Generator(device=dev).manual_seed(5)
  perm = torch.randperm(m, device=dev, generator=g)
  assert torch.equal(perm, runs[0][0].last_permutation)
  per_batch = []
  for g0 in range(0, m, bs):
    idx = perm[g0:g0 + bs]
    rows = (idx.unsqueeze(0).expand(K, -1) if member_rows is None else member_rows[:, idx]).contiguous()
    noise = torch.empty(K, idx.numel(), 4, 2, device=dev).normal_(0.0, 1e-2, generator=g)
    per_batch.append(hand.train_step(cache.feat, cache.vec, target=cache.future, rows=rows, noise=noise))
  assert torch.equal(hand.params, runs[0][0].params) and torch.equal(torch.stack(per_batch), runs[0][0].last_epoch_losses)
  assert torch.equal(torch.rand(4, device=dev, generator=g), torch.rand(4, device=dev, generator=runs[0][1]))


def test_refusals(dev, agents):
  tr = trainer_for(agents(3), max_batch=4)
  feat, vec, y = torch.zeros(3, 4, 128, device=dev), torch.zeros(4, 5, device=dev), torch.zeros(3, 4, 4, 2, device=dev)
  with pytest.raises(RuntimeError, match="no CPU path"):
    tr.backward(feat.cpu(), vec, y=y)
  with pytest.raises(ValueError, match="K=3"):
    tr.backward(feat[:2].contiguous(), vec, y=y)
  with pytest.raises(ValueError, match="max_batch=4"):
    tr.backward(torch.zeros(3, 5, 128, device=dev), torch.zeros(5, 5, device=dev), y=torch.zeros(3, 5, 4, 2, device=dev))
  with pytest.raises(ValueError, match="exactly one"):
    tr.backward(feat, vec)
  with pytest.raises(ValueError, match="int64"):
    tr.backward(feat, vec, y=y, rows=torch.zeros(3, 4, device=dev, dtype=torch.int32))
  with pytest.raises(ValueError, match="num_timesteps_to_keep=4"):
    tr.backward(feat, vec, target=torch.zeros(4, 7, 2, device=dev))
