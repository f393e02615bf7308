"""Ensemble disagreement of plans ("identify" of RIP): `ensemble_stats_kernel` through `rip_plan_stats` / `rip_act_stats`,
`RIPAgent(stats=True)`, `plan_batch(return_stats=True)`, `score_trajectories`, `replay_cache(stats=True)`, `score_cache`.

q[k,b,m] = log_prob_k(y[b,m]) - logabsdet_k(y[b,m]) is checked against the oracle (`O.rip_scores` without a goal, the
bound of `test_g8_scores`: rtol 2e-5, atol 2e-3) and bit for bit against `rip_score`; the statistics against float64
numpy reductions of that q (rtol 1e-5, atol 1e-5).  The (K, B, M) cases are the smallest that take every branch of the
kernel: one model, three waves, a second pass over the span (K = 8), a ragged last workgroup (67 rows, two per
workgroup), M > 1 with a prefix shared inside and cut between workgroups.

Worst errors measured on the MI355X (`pytest -s`):
  q against the oracle: max|dq| 1.14e-5 at q in [-59, -5] (K = 4, B = 67), 0.4 % of atol + rtol |q|; the other cases
    3.8e-6 .. 7.6e-6;  q == rip_score: bit for bit in every case;
  statistics against float64 numpy on the same q: mean within 2.9e-6, variance within 5.4e-6 (variances 0.15 .. 105);
  score_cache against the oracle (fp32 encoder, expert futures, q in [-1564, -5]): max|dq| 9.2e-4, 4.5 % of the bound.
"""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oatomobile_amd import weights as W  # noqa: E402
from tests.helpers import synth_observation  # noqa: E402

CASES = [(1, 1, 1), (3, 5, 1), (4, 67, 1), (8, 3, 1), (4, 3, 7)]
RTOL_Q, ATOL_Q = 2e-5, 2e-3  # test_g8_scores' bound for the same quantity
SENTINEL = -12345.5
_Z, _REFS, _HIP = {}, {}, {}


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def hip_model(seed, dev):
  from oatomobile_amd import ImitativeModel
  if seed not in _HIP:
    _HIP[seed] = ImitativeModel.synthetic(seed).to(dev)
  return _HIP[seed]


def oracle_model(seed):
  from oracle import reference_cpu as O
  if seed not in _REFS:
    _REFS[seed] = O.OracleImitativeModel.from_numpy_state_dict(W.synthetic_state_dict(seed))
  return _REFS[seed]


def oracle_ctx(obs_list):
  from oracle import reference_cpu as O
  lid = torch.stack([torch.from_numpy(o["lidar"]) for o in obs_list]).permute(0, 3, 1, 2).contiguous()
  return dict(
      visual_features=O.transform_visual(lid),
      velocity=torch.stack([torch.from_numpy(np.asarray(o["velocity"], np.float32).reshape(3)) for o in obs_list]),
      is_at_traffic_light=torch.tensor([[float(np.reshape(o["is_at_traffic_light"], -1)[0])] for o in obs_list]),
      traffic_light_state=torch.tensor([[float(np.reshape(o["traffic_light_state"], -1)[0])] for o in obs_list]),
  )


def oracle_z(k, B):
  """z [B,64] of oracle model 900 + k on synth_observation(default_rng(40 + i)), i < B: computed once per model (for the
  largest B asked so far) and shared by every test."""
  from oracle import reference_cpu as O
  if k not in _Z or _Z[k].shape[0] < B:
    obs = [synth_observation(np.random.default_rng(40 + i)) for i in range(B)]
    with torch.no_grad():
      _Z[k] = O.params(oracle_model(900 + k), **oracle_ctx(obs))
  return _Z[k][:B]


def trajectories(B, M, seed=7):
  rng = np.random.default_rng(seed)
  return np.cumsum(np.abs(rng.normal(size=(B, M, 4, 2))) * 1.5, axis=2).astype(np.float32)


def make_agent(K, dev, **kw):
  from oatomobile_amd import RIPAgent
  return RIPAgent(None, algorithm="WCM", models=[hip_model(900 + k, dev) for k in range(K)], **kw)


def plan_stats(agent, z, y, B, M, want_q=True, want_stats=True):
  """`rip_plan_stats` through ctypes -> (q [K,B,M], stats [B,M,4]); an output that is not wanted is passed as NULL and
  comes back as None."""
  from oatomobile_amd import _lib
  K = z.shape[0]
  q = torch.full((K, B, M), SENTINEL, device=z.device) if want_q else None
  st = torch.full((B, M, 4), SENTINEL, device=z.device) if want_stats else None
  _lib.check(_lib.load().rip_plan_stats(agent._handle.raw, _lib.ptr(z), _lib.ptr(y), B, M, _lib.ptr(q), _lib.ptr(st),
                                        _lib.current_stream(z.device)))
  return q, st


@pytest.fixture(scope="module")
def cases(dev):
  """Per (K, B, M): the agent, z, y on the device, one `rip_plan_stats` result and the oracle's scores — computed once."""
  from oracle import reference_cpu as O
  out = {}
  for K, B, M in CASES:
    agent = make_agent(K, dev, max_batch=B)
    zs = [oracle_z(k, B) for k in range(K)]
    y = trajectories(B, M)
    z_d = torch.stack(zs).to(dev).contiguous()
    y_d = torch.from_numpy(y).to(dev)
    q, st = plan_stats(agent, z_d, y_d, B, M)
    with torch.no_grad():
      ref = O.rip_scores([oracle_model(900 + k) for k in range(K)], [z.repeat_interleave(M, 0) for z in zs],
                         torch.from_numpy(y).reshape(B * M, 4, 2), None).numpy().reshape(K, B, M)
    out[(K, B, M)] = dict(agent=agent, z=z_d, y=y_d, q=q, stats=st, ref=ref)
  return out


@pytest.mark.parametrize("K,B,M", CASES)
def test_plan_stats_q_against_the_oracle(cases, K, B, M):
  c = cases[(K, B, M)]
  q, ref = c["q"].cpu().numpy(), c["ref"]
  err = np.abs(q - ref)
  print("rip_plan_stats K=%d B=%d M=%d: q in [%.2f, %.2f], max|dq| = %.3g, max |dq| / (atol + rtol |ref|) = %.3g" %
        (K, B, M, ref.min(), ref.max(), err.max(), (err / (ATOL_Q + RTOL_Q * np.abs(ref))).max()))
  assert np.isfinite(q).all()
  np.testing.assert_allclose(q, ref, rtol=RTOL_Q, atol=ATOL_Q)


@pytest.mark.parametrize("K,B,M", CASES)
def test_plan_stats_q_is_rip_score_bit_for_bit(cases, dev, K, B, M):
  from oatomobile_amd import _lib
  c = cases[(K, B, M)]
  S = torch.full((K, B, M), SENTINEL, device=dev)
  _lib.check(_lib.load().rip_score(c["agent"]._handle.raw, 0, K, _lib.ptr(c["z"]), _lib.ptr(c["y"]), None, B, M, 0, 1.0,
                                   _lib.ptr(S), _lib.current_stream(dev)))
  assert torch.equal(c["q"], S)


@pytest.mark.parametrize("K,B,M", CASES)
def test_plan_stats_reduction(cases, K, B, M):
  c = cases[(K, B, M)]
  q32, st = c["q"].cpu().numpy(), c["stats"].cpu().numpy()
  q = q32.astype(np.float64)
  want = np.stack([q.mean(0), q.var(0, ddof=0), q.min(0), q.max(0)], axis=-1)
  print("stats K=%d B=%d M=%d: variance in [%.3g, %.3g], max|d| mean %.3g var %.3g" %
        (K, B, M, want[..., 1].min(), want[..., 1].max(), np.abs(st[..., 0] - want[..., 0]).max(),
         np.abs(st[..., 1] - want[..., 1]).max()))
  np.testing.assert_allclose(st, want, rtol=1e-5, atol=1e-5)
  np.testing.assert_array_equal(st[..., 2], q32.min(0))
  np.testing.assert_array_equal(st[..., 3], q32.max(0))
  if K == 1:
    assert (st[..., 1] == 0.0).all()
    for slot in (0, 2, 3):
      np.testing.assert_array_equal(st[..., slot], q32[0])
  else:
    assert (st[..., 1] > 0).all()  # distinct members disagree
  # the same bits on every run, and with one output NULL at a time
  q2, st2 = plan_stats(c["agent"], c["z"], c["y"], B, M)
  assert torch.equal(q2, c["q"]) and torch.equal(st2, c["stats"])
  q3, none = plan_stats(c["agent"], c["z"], c["y"], B, M, want_stats=False)
  assert none is None and torch.equal(q3, c["q"])
  none, st3 = plan_stats(c["agent"], c["z"], c["y"], B, M, want_q=False)
  assert none is None and torch.equal(st3, c["stats"])


def batch_inputs(B, dev, first=50):
  obs = [synth_observation(np.random.default_rng(first + i)) for i in range(B)]
  lidar = torch.stack([torch.from_numpy(o["lidar"]) for o in obs]).to(dev)
  vec = torch.tensor([[*o["velocity"], o["is_at_traffic_light"], o["traffic_light_state"]] for o in obs], device=dev)
  goal = torch.stack([torch.from_numpy(o["goal"][:, :2].copy()) for o in obs]).to(dev)
  return obs, lidar, vec, goal


def encode_raw(agent, lidar, vec):
  from oatomobile_amd import _lib
  K, B = len(agent._models), lidar.shape[0]
  z = torch.empty(K, B, 64, device=lidar.device)
  _lib.check(_lib.load().rip_encode_raw(agent._handle.raw, _lib.ptr(lidar), 1, lidar.shape[1], lidar.shape[2], _lib.ptr(vec),
                                        B, 0, K, agent._enc_dtype, _lib.ptr(z), _lib.current_stream(lidar.device)))
  return z


def code_bev(lidar):
  """float32 BEV of synth_observation (levels k / 5) -> (codes uint8, lut [256]) as `replay.pack_cache` codes it."""
  values = torch.unique(lidar)
  lut = torch.full((256,), float("nan"), device=lidar.device)
  lut[:values.numel()] = values
  codes = torch.searchsorted(values, lidar.contiguous()).to(torch.uint8)
  assert torch.equal(lut[codes.long()], lidar)
  return codes, lut


def assert_stats_equal(ps, q, st):
  """PlanStats of device tensors against `rip_plan_stats` outputs q [K,B,1], stats [B,1,4]."""
  assert torch.equal(ps.q, q[:, :, 0])
  for i, field in enumerate((ps.mean, ps.variance, ps.min, ps.max)):
    assert field.shape == (q.shape[1],)
    assert torch.equal(field, st[:, 0, i])


@pytest.mark.parametrize("kernel", ["chain", "split"])
@pytest.mark.parametrize("B", [1, 3])
def test_plan_batch_return_stats(dev, kernel, B):
  from oatomobile_amd import PlanStats
  from oatomobile_amd.agents import interpolate_plan
  K, N = 4, 16
  kw = dict(num_candidates=N, seed=3, max_batch=3, search_kernel=kernel)
  plain, agent = make_agent(K, dev, **kw), make_agent(K, dev, stats=True, **kw)
  _, lidar, vec, goal = batch_inputs(B, dev)
  plan0, loss0 = plain.plan_batch(lidar, vec, goal, return_loss=True)
  for a in (agent, plain):  # return_stats works whether or not the agent was built with stats=True
    plan, loss, ps = a.plan_batch(lidar, vec, goal, return_loss=True, return_stats=True)
    assert isinstance(ps, PlanStats)
    assert torch.equal(plan, plan0) and torch.equal(loss, loss0)
    z = encode_raw(a, lidar, vec)
    q, st = plan_stats(a, z, plan.view(B, 1, 4, 2), B, 1)
    assert_stats_equal(ps, q, st)
    assert (ps.variance > 0).all() and torch.isfinite(ps.q).all()
    # interpolate=True: the [B,4,2] plan lives in handle scratch; same statistics, today's interpolated plans
    p30_0 = plain.plan_batch(lidar, vec, goal, interpolate=True)
    p30, ps30 = a.plan_batch(lidar, vec, goal, interpolate=True, return_stats=True)
    assert torch.equal(p30, p30_0)
    np.testing.assert_array_equal(p30[0].cpu().numpy(), interpolate_plan(plan0[0].cpu().numpy()))
    assert_stats_equal(ps30, q, st)
    # the coded entry point
    codes, lut = code_bev(lidar)
    for interp, want in ((False, plan0), (True, p30_0)):
      pc0 = plain.plan_batch_coded(codes, lut, vec, goal, interpolate=interp)
      pc, psc = a.plan_batch_coded(codes, lut, vec, goal, interpolate=interp, return_stats=True)
      assert torch.equal(pc, pc0) and torch.equal(pc, want)
      assert_stats_equal(psc, q, st)


def test_online_call_reports_stats(dev):
  """`agent(observation)` with `stats=True`: one captured graph, the plan of a `stats=False` agent, `last_stats` equal to
  the batch path; the weight snapshot (and with it the statistics) follows `load_numpy_state_dict`."""
  from oatomobile_amd import ImitativeModel, PlanStats, RIPAgent
  models = [ImitativeModel.synthetic(810 + k).to(dev) for k in range(2)]
  kw = dict(algorithm="MA", models=models, num_candidates=16, seed=2, graph=True)
  s_agent, p_agent = RIPAgent(None, stats=True, **kw), RIPAgent(None, **kw)
  assert s_agent.last_stats is None and p_agent.last_stats is None

  def batch_stats(ob):
    lidar = torch.from_numpy(ob["lidar"]).to(dev)[None]
    vec = torch.tensor([[*ob["velocity"], ob["is_at_traffic_light"], ob["traffic_light_state"]]], device=dev)
    goal = torch.from_numpy(ob["goal"][None, :, :2].copy()).to(dev)
    return s_agent.plan_batch(lidar, vec, goal, return_stats=True)[1]

  def check(ob):
    a, b = s_agent(dict(ob)), p_agent(dict(ob))
    np.testing.assert_array_equal(a, b)
    got, want = s_agent.last_stats, batch_stats(ob)
    assert isinstance(got, PlanStats) and got.q.shape == (2, 1) and got.mean.shape == (1,)
    for g, w in zip(got, want):
      assert isinstance(g, np.ndarray)
      np.testing.assert_array_equal(g, w.cpu().numpy())
    return got

  seen = []
  for i in range(4):
    seen.append(check(synth_observation(np.random.default_rng(30 + i))))
  assert len({float(s.variance[0]) for s in seen}) == 4  # refreshed call after call
  st = next(iter(s_agent._online.values()))
  assert st["graph"] is not None
  assert p_agent.last_stats is None
  ob = synth_observation(np.random.default_rng(33))
  before = seen[-1]
  models[1].load_numpy_state_dict(W.synthetic_state_dict(999))
  after = check(ob)
  assert after.q[0, 0] != before.q[0, 0] or after.q[1, 0] != before.q[1, 0]
  assert after.variance[0] != before.variance[0]
  assert p_agent.last_stats is None


@pytest.fixture(scope="module")
def packed(tmp_path_factory, dev):
  """8 datums with targets, packed the way tests/test_train_epoch.py packs its caches."""
  from oatomobile_amd import replay
  from tests.test_train_epoch import write_datums
  root = tmp_path_factory.mktemp("plan_stats")
  files = write_datums(str(root / "d"), 8, seed=6)
  cache = replay.pack_cache(files, str(root / "d_cache"), workers=1, targets=True)
  return files, cache


def test_replay_cache_stats(packed, dev):
  from oatomobile_amd import replay
  _, cache = packed
  K = 4
  agent = make_agent(K, dev, num_candidates=16, seed=1, max_batch=3)
  plans0 = replay.replay_cache(agent, cache, 3)
  res1 = replay.replay_cache(agent, cache, 3, stats=True)
  res2 = replay.replay_cache(agent, cache, 3, stats=True, streams=2)
  plans, stats, q = res1
  assert plans.shape == (8, 4, 2) and stats.shape == (8, 4) and q.shape == (8, K)
  assert stats.dtype == np.float32 and q.dtype == np.float32
  np.testing.assert_array_equal(plans, plans0)
  for a, b in zip(res1, res2):
    np.testing.assert_array_equal(a, b)
  lut = torch.from_numpy(cache.lut).to(dev)
  for i0 in range(0, 8, 3):
    rows = slice(i0, min(i0 + 3, 8))
    codes = torch.from_numpy(np.array(cache.codes[rows])).to(dev)
    vec, goal = torch.from_numpy(np.array(cache.vec[rows])).to(dev), torch.from_numpy(np.array(cache.goal[rows])).to(dev)
    p, ps = agent.plan_batch_coded(codes, lut, vec, goal, return_stats=True)
    np.testing.assert_array_equal(plans[rows], p.cpu().numpy())
    np.testing.assert_array_equal(q[rows], ps.q.t().cpu().numpy())
    np.testing.assert_array_equal(stats[rows], torch.stack(tuple(ps[1:]), dim=1).cpu().numpy())
  assert (stats[:, 1] > 0).all()
  p30, stats30, q30 = replay.replay_cache(agent, cache, 3, interpolate=True, stats=True)
  assert p30.shape == (8, 30, 3)
  np.testing.assert_array_equal(stats30, stats)
  np.testing.assert_array_equal(q30, q)


def test_score_cache_and_score_trajectories(packed, dev):
  from oatomobile_amd import replay
  from oatomobile_amd._datum import load_datum
  from oracle import reference_cpu as O
  files, cache = packed
  files, n, K = files[:6], 6, 3
  data = replay.DeviceCache(replay.pack_cache(files, cache.dir + "_six", workers=1, targets=True), dev)
  agent = make_agent(K, dev, max_batch=4)
  res = replay.score_cache(agent, data, 4)  # batches of 4 and 2
  assert res["q"].shape == (n, K) and res["stats"].shape == (n, 4) and res["q"].dtype == np.float32
  datums = [load_datum(f) for f in files]
  L = datums[0]["player_future"].shape[0]
  expert = np.stack([d["player_future"][0::L // 4, :2] for d in datums]).astype(np.float32)  # [n,4,2]
  assert expert.shape == (n, 4, 2)
  with torch.no_grad():
    ctx = oracle_ctx(datums)
    zs = [O.params(oracle_model(900 + k), **ctx) for k in range(K)]
    ref = O.rip_scores([oracle_model(900 + k) for k in range(K)], zs, torch.from_numpy(expert), None).numpy()  # [K,n]
  err = np.abs(res["q"] - ref.T)
  print("score_cache: q in [%.2f, %.2f], max|dq| = %.3g, max |dq| / (atol + rtol |ref|) = %.3g" %
        (ref.min(), ref.max(), err.max(), (err / (ATOL_Q + RTOL_Q * np.abs(ref.T))).max()))
  np.testing.assert_allclose(res["q"], ref.T, rtol=RTOL_Q, atol=ATOL_Q)
  q64 = res["q"].astype(np.float64)
  np.testing.assert_allclose(res["stats"], np.stack([q64.mean(1), q64.var(1), q64.min(1), q64.max(1)], axis=1),
                             rtol=1e-5, atol=1e-5)
  # score_trajectories: M = 1 and M = 3 against rip_plan_stats on the same handle's z, bit for bit
  B = 4
  lidar = torch.from_numpy(np.stack([d["lidar"] for d in datums[:B]])).to(dev)
  vec = torch.from_numpy(np.array(cache.vec[:B])).to(dev)
  z = encode_raw(agent, lidar, vec)
  y1 = torch.from_numpy(expert[:B]).to(dev)
  ps = agent.score_trajectories(lidar, vec, y1)
  q, st = plan_stats(agent, z, y1.view(B, 1, 4, 2), B, 1)
  assert_stats_equal(ps, q, st)
  np.testing.assert_allclose(ps.q.t().cpu().numpy(), res["q"][:B], rtol=RTOL_Q, atol=ATOL_Q)  # raw BEV vs gathered batch
  y3 = torch.from_numpy(trajectories(B, 3, seed=11)).to(dev)
  ps3 = agent.score_trajectories(lidar, vec, y3)
  q, st = plan_stats(agent, z, y3, B, 3)
  assert ps3.q.shape == (K, B, 3) and ps3.variance.shape == (B, 3)
  assert torch.equal(ps3.q, q)
  for i, field in enumerate(ps3[1:]):
    assert torch.equal(field, st[..., i])
  # the dtype / device / shape checks of plan_batch
  with pytest.raises(ValueError, match="float32"):
    agent.score_trajectories(lidar, vec, y1.double())
  with pytest.raises(RuntimeError, match="must be a tensor on"):
    agent.score_trajectories(lidar, vec, y1.cpu())
  with pytest.raises(ValueError, match="y must have shape"):
    agent.score_trajectories(lidar, vec, y1[:, :3])
  with pytest.raises(ValueError, match="y must have shape"):
    agent.score_trajectories(lidar, vec, y3[:2])
  with pytest.raises(ValueError, match="max_batch"):
    agent.score_trajectories(lidar.repeat(2, 1, 1, 1), vec.repeat(2, 1), y1.repeat(2, 1, 1))


def test_abi_validation(dev):
  from oatomobile_amd import _lib
  lib = _lib.load()
  K, B, M = 2, 2, 2
  agent = make_agent(K, dev, num_candidates=4, max_batch=B)
  h = agent._handle.raw
  z = torch.stack([oracle_z(k, B) for k in range(K)]).to(dev).contiguous()
  y = torch.from_numpy(trajectories(B, M)).to(dev)
  q = torch.full((K, B, M), SENTINEL, device=dev)
  st = torch.full((B, M, 4), SENTINEL, device=dev)
  stream = _lib.current_stream(dev)
  null = ctypes.c_void_p(0)
  bad = [("handle", (null, _lib.ptr(z), _lib.ptr(y), B, M, _lib.ptr(q), _lib.ptr(st))),
         ("z_dev", (h, null, _lib.ptr(y), B, M, _lib.ptr(q), _lib.ptr(st))),
         ("y_dev", (h, _lib.ptr(z), null, B, M, _lib.ptr(q), _lib.ptr(st))),
         ("B=0", (h, _lib.ptr(z), _lib.ptr(y), 0, M, _lib.ptr(q), _lib.ptr(st))),
         ("M=-1", (h, _lib.ptr(z), _lib.ptr(y), B, -1, _lib.ptr(q), _lib.ptr(st))),
         ("q_dev and stats_dev", (h, _lib.ptr(z), _lib.ptr(y), B, M, null, null))]
  for name, args in bad:
    assert lib.rip_plan_stats(*args, stream) == _lib.RIP_EINVAL, name
    assert name in lib.rip_last_error().decode(), (name, lib.rip_last_error())
  torch.cuda.synchronize(dev)
  assert (q == SENTINEL).all() and (st == SENTINEL).all()  # nothing was launched
  assert lib.rip_plan_stats(h, _lib.ptr(z), _lib.ptr(y), B, M, _lib.ptr(q), _lib.ptr(st), stream) == 0
  assert (q != SENTINEL).all() and (st != SENTINEL).all()
  # rip_act_stats with both extra pointers NULL is rip_act
  _, lidar, vec, goal = batch_inputs(B, dev)
  common = (h, _lib.ptr(lidar), 1, 200, 200, _lib.ptr(vec), _lib.ptr(goal), _lib.ptr(agent._x0(B)), B, 4, goal.shape[1],
            _lib.ALGORITHMS["WCM"], 10, 0.1, 1.0, 0)
  plan_a, plan_b = torch.empty(B, 4, 2, device=dev), torch.empty(B, 4, 2, device=dev)
  loss_a, loss_b = torch.empty(B, 4, device=dev), torch.empty(B, 4, device=dev)
  _lib.check(lib.rip_act(*common, _lib.ptr(plan_a), _lib.ptr(loss_a), None, stream))
  _lib.check(lib.rip_act_stats(*common, _lib.ptr(plan_b), _lib.ptr(loss_b), None, None, None, stream))
  assert torch.equal(plan_a, plan_b) and torch.equal(loss_a, loss_b)
  q1, st1 = torch.full((K, B), SENTINEL, device=dev), torch.full((B, 4), SENTINEL, device=dev)
  _lib.check(lib.rip_act_stats(*common, _lib.ptr(plan_b), _lib.ptr(loss_b), None, _lib.ptr(q1), None, stream))
  _lib.check(lib.rip_act_stats(*common, _lib.ptr(plan_b), None, None, None, _lib.ptr(st1), stream))
  assert torch.equal(plan_a, plan_b) and torch.equal(loss_a, loss_b)
  assert (q1 != SENTINEL).all() and (st1 != SENTINEL).all()
  np.testing.assert_allclose(st1[:, 0].cpu().numpy(), q1.double().mean(0).cpu().numpy(), rtol=1e-5, atol=1e-5)
  # without a plan output there is nothing to act on, as in rip_act
  assert lib.rip_act_stats(*common, None, None, None, _lib.ptr(q1), _lib.ptr(st1), stream) == _lib.RIP_EINVAL


def test_kernel_log_is_unchanged_by_the_stats_flag(dev):
  """With `stats` off (and on: the statistics launch is not an encoder kernel) an agent's encoder launch list is the
  same; `rip_kernel_log` of two agents that differ only in the flag agree."""
  from oatomobile_amd import _lib
  logs = []
  _, lidar, vec, goal = batch_inputs(2, dev)
  for stats in (False, True):
    agent = make_agent(2, dev, num_candidates=4, max_batch=2, stats=stats)
    agent._handle.set_option(_lib.OPT_KERNEL_LOG, 1)
    agent.plan_batch(lidar, vec, goal, return_stats=stats)
    logs.append(agent._handle.kernel_log())
  assert logs[0] and logs[0] == logs[1]
