"""Handing a trainer's weights to a live RIPAgent on the device: `rip_load_model_device` (csrc/weights_pack.hip) against
`rip_load_model`, `RIPAgent.load_member` against `sync_to_model()` + `refresh()`.  Every comparison is bit equality: the
host packers are the reference, and the device path repeats their arithmetic operation for operation."""

import numpy as np
import pytest
import torch

from tests.helpers import synth_observation

pytestmark = pytest.mark.gpu

K, MAX_BATCH, B, N, G, TRAIN_B = 2, 4, 2, 16, 3, 3
BUFFERS = ("enc_w", "enc_wh", "enc_wt", "enc_wc", "enc_wr", "flow_w", "mfma_w", "split_w")
PW = "_encoder._model.features.8.conv.0.0.weight"   # [384, 64, 1, 1]: the expansion of a split-f16 tile block
PW_BN = "_encoder._model.features.8.conv.0.1."
BN_EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  torch.cuda.set_device(0)
  return torch.device("cuda", 0)


def packed_of(sd, C):
  from oatomobile_amd import weights
  return weights.pack_state_dict(sd, C)


def state_dict(seed, C):
  from oatomobile_amd import weights
  return weights.synthetic_state_dict(seed, C)


def handle(C, packs):
  """A K = 2 handle with `packs[k]` (numpy, or None) loaded through `rip_load_model`."""
  from oatomobile_amd import _lib
  h = _lib.Handle(K, C, MAX_BATCH, 0, max_candidates=N)
  for k, p in enumerate(packs):
    if p is not None:
      h.load_model(k, p)
  return h


def slices(h, k):
  return [h.peek_weights(k, which) for which in range(len(BUFFERS))]


def flag_bits(h, k):
  wmax, ok = h.model_flags(k)
  return int(np.float32(wmax).view(np.uint32)), ok


def assert_slot_equal(a, b, what):
  for name, x, y in zip(BUFFERS, a, b):
    assert x.numel() == y.numel() and x.numel() > 0, (what, name)
    if not torch.equal(x, y):
      bad = torch.nonzero(x != y).flatten()
      raise AssertionError("%s: %s differs in %d of %d bytes, first at byte %d" % (what, name, bad.numel(), x.numel(), int(bad[0])))


def trained_params(C, dev, seed):
  """The packed parameters of a DIMTrainer after two real train steps (running statistics have moved)."""
  from tests.test_train_deterministic import dim_case
  from oatomobile_amd import DIMTrainer, ImitativeModel
  tr = DIMTrainer(ImitativeModel.synthetic(seed, in_channels=C).to(dev), lr=1e-3, max_batch=MAX_BATCH, device=dev)
  for step in range(2):
    batch, kw = dim_case(TRAIN_B, C, dev, 900 + step)
    tr.train_step(batch, **kw)
  return tr


def folded(sd, key, bn):
  """fold_and_pack's arithmetic for one conv in numpy: float32(float64(w) * (gamma / sqrt(var + eps)))."""
  scale = sd[bn + "weight"].astype(np.float64) / np.sqrt(sd[bn + "running_var"].astype(np.float64) + BN_EPS)
  return (sd[key].astype(np.float64) * scale.reshape(-1, 1, 1, 1)).astype(np.float32)


def edge_state_dict(seed, C):
  """Weights at the edges of the operand formats, in one pointwise layer and in the flow: 0, values whose 2^8 multiple is a binary16
  subnormal (1e-8: below half the smallest one, 6e-8), a folded magnitude just under SPLIT_ENC_W_LIMIT = 240; one
  BatchNorm channel with running_var 0 (scale = gamma / sqrt(eps)) and one with weight 0 (signed zeros)."""
  sd = state_dict(seed, C)
  w = sd[PW]
  for c in (0, 1):
    sd[PW_BN + "weight"][c] = 1.0
    sd[PW_BN + "running_var"][c] = 1.0
  w[0, :5, 0, 0] = [0.0, 1e-8, -1e-8, 6e-8, -6e-8]
  w[1, 0, 0, 0] = np.float32(239.99 * np.sqrt(1.0 + BN_EPS))
  w[1, 1, 0, 0] = -w[1, 0, 0, 0]
  sd[PW_BN + "running_var"][2] = 0.0
  sd[PW_BN + "weight"][3] = 0.0
  # the flow's operands are split into binary16 terms as well: signed zeros and 2^8 multiples in the subnormal range
  for key in ("_decoder._decoder.weight_ih", "_decoder._decoder.weight_hh", "_decoder._locscale._model.0.weight",
              "_decoder._locscale._model.2.weight"):
    sd[key][1, :5] = np.array([-0.0, 1e-8, -1e-8, 6e-8, -6e-8], np.float32)[:sd[key].shape[1]]
  f = np.abs(folded(sd, PW, PW_BN))
  assert 239.9 < f[1, 0, 0, 0] < 240.0 and f.max() < 240.0, (f[1, 0, 0, 0], f.max())
  return sd


@pytest.fixture(scope="module")
def observations(dev):
  out = {}
  for C in (2, 3):
    obs = [synth_observation(np.random.default_rng(7400 + i), C=C, G=G) for i in range(B)]
    lidar = torch.stack([torch.from_numpy(o["lidar"]) for o in obs]).to(dev)
    vec = torch.tensor([[*o["velocity"], o["is_at_traffic_light"], o["traffic_light_state"]] for o in obs], device=dev)
    goal = torch.stack([torch.from_numpy(o["goal"][:, :2].copy()) for o in obs]).to(dev)
    out[C] = (obs, lidar.float().contiguous(), vec.float().contiguous(), goal.float().contiguous())
  return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. bytes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["seed", "trained", "edges"])
@pytest.mark.parametrize("C", [2, 3])
def test_device_load_writes_the_bytes_of_the_host_load(dev, C, source):
  s1 = packed_of(state_dict(610, C), C)
  if source == "seed":
    dev_vec = torch.from_numpy(packed_of(state_dict(611, C), C)).to(dev)
  elif source == "trained":
    dev_vec = trained_params(C, dev, 611).params
  else:
    dev_vec = torch.from_numpy(packed_of(edge_state_dict(611, C), C)).to(dev)
  s2 = dev_vec.cpu().numpy()
  a, b = handle(C, [s1, s1]), handle(C, [None, s2])
  slot0 = slices(a, 0)
  a.load_model_device(1, dev_vec)
  assert_slot_equal(slices(a, 1), slices(b, 1), "C=%d %s: slot 1" % (C, source))
  assert_slot_equal(slices(a, 0), slot0, "C=%d %s: slot 0 (not loaded)" % (C, source))
  assert flag_bits(a, 1) == flag_bits(b, 1)
  if source == "edges":
    assert flag_bits(a, 1)[1] is True  # just under the limit: still inside
  a.close()
  b.close()


def test_argument_errors_on_a_live_handle(dev):
  """The checks that need a handle (tests/test_publish_cpu.py has those that do not): nothing is launched, the slot
  stays as it was."""
  from oatomobile_amd import _lib, arch
  lib = _lib.load()
  vec = torch.from_numpy(packed_of(state_dict(611, 2), 2)).to(dev)
  h = handle(2, [packed_of(state_dict(610, 2), 2), None])
  before = slices(h, 0)
  n = arch.packed_numel(2)
  size = _lib.c_size_t(0)
  for call, word in (
      (lambda: lib.rip_load_model_device(h.raw, K, _lib.ptr(vec), n, None), "model index"),
      (lambda: lib.rip_load_model_device(h.raw, -1, _lib.ptr(vec), n, None), "model index"),
      (lambda: lib.rip_load_model_device(h.raw, 0, _lib.ptr(vec), n - 1, None), "wrong length"),
      (lambda: lib.rip_load_model_device(h.raw, 0, _lib.ptr(vec), n + 1, None), "wrong length"),
      (lambda: lib.rip_load_model_device(h.raw, 0, None, n, None), "NULL"),
      (lambda: lib.rip_peek_weights(h.raw, K, 0, None, 0, _lib.ctypes.byref(size), None), "model index"),
      (lambda: lib.rip_peek_weights(h.raw, 0, 8, None, 0, _lib.ctypes.byref(size), None), "unknown weight buffer"),
      (lambda: lib.rip_peek_weights(h.raw, 0, 0, _lib.ptr(vec), 16, None, None), "cap_bytes"),
      (lambda: lib.rip_model_flags(h.raw, K, None, None), "model index"),
  ):
    assert call() == _lib.RIP_EINVAL
    assert word in lib.rip_last_error().decode(), lib.rip_last_error()
  assert lib.rip_model_flags(h.raw, 1, None, None) == _lib.RIP_ESTATE  # nothing loaded there
  assert lib.rip_peek_weights(h.raw, 1, 0, _lib.ptr(vec), vec.numel() * 4, None, None) == _lib.RIP_ESTATE
  with pytest.raises(ValueError):
    h.load_model_device(0, vec[:-1])
  with pytest.raises(ValueError):
    h.load_model_device(0, vec.cpu())
  assert_slot_equal(slices(h, 0), before, "slot 0 after refused calls")
  h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. routing: the two flags select kernels
# ---------------------------------------------------------------------------------------------------------------------
def out_of_range_state_dict(which, seed=611, C=2):
  sd = state_dict(seed, C)
  if which == "flow":
    sd["_decoder._decoder.weight_hh"][0, 0] = 300.0  # >= SPLIT_W_LIMIT
  elif which == "encoder":
    sd[PW_BN + "weight"][5] = 1.0
    sd[PW_BN + "running_var"][5] = 1.0
    sd[PW][5, 5, 0, 0] = 500.0
    assert abs(folded(sd, PW, PW_BN)[5, 5, 0, 0]) > 240.0
  else:
    sd["_decoder._locscale._model.0.weight"][0, 0] = np.nan
  return sd


@pytest.mark.parametrize("which", ["flow", "encoder", "nan"])
def test_flags_route_as_after_a_host_load(dev, observations, which):
  from oatomobile_amd import _lib
  lib = _lib.load()
  C = 2
  _, lidar, vec, goal = observations[C]
  s1, s2 = packed_of(state_dict(610, C), C), packed_of(out_of_range_state_dict(which), C)
  a, b = handle(C, [s1, s1]), handle(C, [s1, s2])
  assert flag_bits(a, 1) == (flag_bits(a, 0)[0], True)
  a.load_model_device(1, torch.from_numpy(s2).to(dev))
  assert flag_bits(a, 1) == flag_bits(b, 1)
  assert flag_bits(a, 1) != flag_bits(a, 0)
  x0 = torch.randn(B, N, 4, 2, generator=torch.Generator().manual_seed(3)).to(dev)
  res = []
  for h in (a, b):
    plan = (_lib.c_int32 * 10)()
    _lib.check(lib.rip_search_plan(h.raw, 80, 16, plan, 10))
    h.set_option(_lib.OPT_KERNEL_LOG, 1)
    z = torch.empty(K, B, 64, device=dev)
    _lib.check(lib.rip_encode_raw(h.raw, _lib.ptr(lidar), 1, lidar.shape[1], lidar.shape[2], _lib.ptr(vec), B, 0, K, 0, _lib.ptr(z),
                                  h.stream()))
    log = h.kernel_log()
    plans = torch.empty(B, N, 4, 2, device=dev)
    if which != "nan":
      _lib.check(lib.rip_search(h.raw, _lib.ptr(z), _lib.ptr(goal), _lib.ptr(x0), B, N, G, 0, 10, 0.1, 1.0, None, _lib.ptr(plans),
                                None, None, None, None, None, h.stream()))
    res.append((list(plan), log, z, plans))
  assert res[0][0] == res[1][0] and res[0][0][0] == (4 if which == "encoder" else 3)
  assert res[0][1] == res[1][1] and len(res[0][1]) > 0
  if which != "nan":
    assert torch.isfinite(res[0][2]).all() and torch.equal(res[0][2], res[1][2])
    assert torch.equal(res[0][3].view(torch.int32), res[1][3].view(torch.int32))
  a.close()
  b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the agent, both roads
# ---------------------------------------------------------------------------------------------------------------------
def make_models(dev, C=2):
  from oatomobile_amd import ImitativeModel
  return [ImitativeModel.synthetic(620 + k, in_channels=C).to(dev) for k in range(K)]


def train_member(models, k, dev, C=2):
  from tests.test_train_deterministic import dim_case
  from oatomobile_amd import DIMTrainer
  tr = DIMTrainer(models[k], lr=1e-3, max_batch=MAX_BATCH, device=dev)
  for step in range(2):
    batch, kw = dim_case(TRAIN_B, C, dev, 910 + step)
    tr.train_step(batch, **kw)  # (ends with apply(): the next call on this stream follows it with no synchronise)
  return tr


@pytest.mark.parametrize("search_kernel", ["chain", "phase", "split"])
@pytest.mark.parametrize("encoder_dtype", ["fp32", "bf16"])
def test_load_member_plans_like_sync_and_refresh(dev, observations, encoder_dtype, search_kernel):
  from oatomobile_amd import RIPAgent
  _, lidar, vec, goal = observations[2]
  models = make_models(dev)
  kw = dict(algorithm="WCM", models=models, num_candidates=N, max_batch=MAX_BATCH, seed=2, encoder_dtype=encoder_dtype,
            search_kernel=search_kernel)
  host, device = RIPAgent(None, **kw), RIPAgent(None, **kw)
  before = host.plan_batch(lidar, vec, goal)
  tr = train_member(models, 1, dev)
  device.load_member(1, tr)  # road 2 first: the model objects still hold the old weights
  got = device.plan_batch(lidar, vec, goal, return_loss=True, return_stats=True)
  tr.sync_to_model()  # road 1
  host.refresh()
  want = host.plan_batch(lidar, vec, goal, return_loss=True, return_stats=True)
  assert not torch.equal(want[0], before), "training did not change the plans"
  assert torch.isfinite(want[0]).all()
  assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
  assert torch.equal(got[2].q, want[2].q)
  for name in ("mean", "variance", "min", "max"):
    assert torch.equal(getattr(got[2], name), getattr(want[2], name)), name


def test_publish_and_load_members(dev, observations):
  from oatomobile_amd import RIPAgent
  _, lidar, vec, goal = observations[2]
  models = make_models(dev)
  kw = dict(algorithm="MA", models=models, num_candidates=N, max_batch=MAX_BATCH, seed=2)
  one, two = RIPAgent(None, **kw), RIPAgent(None, **kw)
  tr = train_member(models, 0, dev)
  tr.publish(one, 0)
  two.load_members([tr.params, None])
  assert torch.equal(one.plan_batch(lidar, vec, goal), two.plan_batch(lidar, vec, goal))
  with pytest.raises(ValueError):
    two.load_members([tr])
  with pytest.raises(ValueError):
    two.load_member(K, tr)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the captured one-observation pipeline survives a load
# ---------------------------------------------------------------------------------------------------------------------
def test_captured_pipeline_survives_a_load(dev, observations):
  from oatomobile_amd import ImitativeModel, RIPAgent
  obs = observations[2][0]
  models = make_models(dev)
  kw = dict(algorithm="WCM", num_candidates=N, seed=2)
  agent = RIPAgent(None, models=models, **kw)
  first = agent(dict(obs[0]))
  (key, captured), = agent._online.items()
  tr = train_member(models, 1, dev)
  agent.load_member(1, tr)
  plan = agent(dict(obs[0]))
  assert agent._online[key] is captured, "the captured pipeline was dropped although no flag changed"
  tr.sync_to_model()
  np.testing.assert_array_equal(plan, RIPAgent(None, models=models, **kw)(dict(obs[0])))
  assert np.abs(plan - first).max() > 0
  agent(dict(obs[0]))  # (the model changed: the host road runs and re-captures)
  # a member outside the split-f16 search's operand range: kernel selection changes, so the capture goes
  sd = out_of_range_state_dict("flow", seed=621)
  agent.load_member(1, torch.from_numpy(packed_of(sd, 2)).to(dev))
  assert agent._online == {}
  other = [models[0], ImitativeModel(in_channels=2).load_numpy_state_dict(sd).to(dev)]
  np.testing.assert_array_equal(agent(dict(obs[1])), RIPAgent(None, models=other, **kw)(dict(obs[1])))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the replay twin follows; refresh() goes back to the model objects
# ---------------------------------------------------------------------------------------------------------------------
def test_twin_follows_and_refresh_goes_back(dev, tmp_path):
  from oatomobile_amd import RIPAgent, replay
  models = make_models(dev)
  kw = dict(algorithm="MA", models=models, num_candidates=8, max_batch=3, seed=4)
  agent = RIPAgent(None, **kw)
  ep = replay.Episode(str(tmp_path), "ep")
  rng = np.random.default_rng(5)
  for i in range(6):
    o = synth_observation(np.random.default_rng(8400 + i))
    fut = np.cumsum(np.abs(rng.normal(size=(80, 3))) * 0.4, axis=0).astype(np.float32)
    ep.append("f%02d" % i, lidar=o["lidar"], velocity=o["velocity"], is_at_traffic_light=o["is_at_traffic_light"],
              traffic_light_state=o["traffic_light_state"], player_future=fut)
  cache = replay.pack_cache(ep.files(), str(tmp_path / "cache"))
  built = replay.replay_cache(agent, cache, 3, streams=2)  # (creates the twin)
  assert agent._replay_twin is not None
  tr = train_member(models, 1, dev)
  agent.load_member(1, tr)
  one, two = replay.replay_cache(agent, cache, 3), replay.replay_cache(agent, cache, 3, streams=2)
  np.testing.assert_array_equal(two, one)
  assert np.abs(one - built).max() > 0, "training did not change the plans"
  agent.refresh()
  np.testing.assert_array_equal(replay.replay_cache(agent, cache, 3, streams=2), built)
  np.testing.assert_array_equal(replay.replay_cache(agent, cache, 3), built)
  tr.sync_to_model()
  np.testing.assert_array_equal(replay.replay_cache(agent, cache, 3, streams=2), one)
