"""Sample-and-rank ensemble prediction: `rip_sample_normal`, `rip_predict` (`sample_forward_kernel`, the statistics launch,
`rank_kernel`), `RIPAgent.predict_batch` / `predict_batch_coded`, `replay.predict_cache`.

Models, z and observations are those of tests/test_plan_stats.py (members 900 + k, the oracle's z).  The (K, S, B, top_k)
cases: the smallest shape; odd sizes; K = 8 (a second member pass in the scorer); 67 observations (a ragged grid);
M = 268 candidates (more than the ranking workgroup's 256 threads) with top_k at its cap of 64; top_k = M (a full sort).

Bounds.  The device generator against its numpy restatement: |d| <= 1e-5 — both evaluate the same fp32 expressions with
different libms; the angle 2 pi v <= 6.28 carries half an ulp (2.4e-7) from its rounding, sincosf and logf / sqrtf are
good to a few ulp, and the radius is at most 5.77, which gives about 5.5e-6.  y_all against the oracle's flow: atol 1e-4
(test_g2_flow).  q against the oracle: rtol 2e-5, atol 2e-3 (test_plan_stats.py).  The goal term: rtol 1e-5, atol 2e-4
(test_g4_goal).  ade / fde against float64 numpy: atol 1e-5.  Everything else is exact.

Worst values measured on the MI355X (`pytest -s`) are in the docstrings of the tests.
"""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oatomobile_amd import prediction  # noqa: E402
from tests.test_plan_stats import (ATOL_Q, RTOL_Q, batch_inputs, code_bev, hip_model, make_agent, oracle_model, oracle_z,  # noqa: E402
                                   plan_stats)

CASES = [(1, 1, 1, 1), (3, 5, 2, 4), (8, 3, 3, 5), (2, 2, 67, 1), (4, 67, 2, 64), (2, 3, 1, 6)]
ALGOS = {"WCM": 0, "MA": 1, "BCM": 2}
SENTINEL = -12345.5
EPS = 0.75  # of the goal likelihood
KNOWN_NORMALS = {
    0: [-0.11691724, 0.99785749, 0.15243754, 0.08834561, -1.05520091, -1.14492148, 0.53078726, 1.14905974],
    2**32 + 5: [0.61690571, 0.86306567, -0.27411423, -0.54956671, -0.03821556, 0.21167508, -0.14071117, 1.28665505],
}


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def sample_normal(seed, first_id, n, dev):
  from oatomobile_amd import _lib
  out = torch.full((n, 8), SENTINEL, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().rip_sample_normal(seed, first_id, n, _lib.ptr(out), _lib.current_stream(dev)))
  return out.cpu().numpy()


def predict(agent, z, S, top_k, algorithm="WCM", noise=None, goal=None, target=None, seed=0, row0=0, want_loss_all=True):
  """`rip_predict` through ctypes into sentinel-filled buffers -> dict of device tensors (and the return code)."""
  from oatomobile_amd import _lib
  K, B = z.shape[0], z.shape[1]
  M, dev = K * S, z.device
  full = lambda *shape: torch.full(shape, SENTINEL, device=dev)  # noqa: E731
  o = dict(y_all=full(B, M, 4, 2), q=full(K, B, M), stats=full(B, M, 4), loss_all=full(B, M) if want_loss_all else None,
           y_top=full(B, top_k, 4, 2), loss_top=full(B, top_k), index_top=torch.full((B, top_k), -7, device=dev, dtype=torch.int32),
           ade=full(B, top_k) if target is not None else None, fde=full(B, top_k) if target is not None else None)
  o["rc"] = _lib.load().rip_predict(
      agent._handle.raw, _lib.ptr(z), _lib.ptr(goal), 0 if goal is None else goal.shape[1], EPS, _lib.ptr(target), _lib.ptr(noise),
      seed, row0, B, S, top_k, ALGOS[algorithm], _lib.ptr(o["y_all"]), _lib.ptr(o["q"]), _lib.ptr(o["stats"]),
      _lib.ptr(o["loss_all"]), _lib.ptr(o["y_top"]), _lib.ptr(o["loss_top"]), _lib.ptr(o["index_top"], torch.int32),
      _lib.ptr(o["ade"]), _lib.ptr(o["fde"]), _lib.current_stream(dev))
  return o


def numpy_loss(q, algorithm):
  """aggregate_scores_kernel's convention on q [K,B,M] in float32."""
  if algorithm == "WCM":
    return (-q).min(0)
  if algorithm == "BCM":
    return (-q).max(0)
  return ((-q).astype(np.float64).mean(0)).astype(np.float32)


@pytest.fixture(scope="module")
def cases(dev):
  """Per (K, S, B, top_k): the agent, z, a noise tensor, a goal and a target, and ONE `rip_predict` on the noise (WCM, no
  goal, with the target) — shared by the tests below."""
  out = {}
  for K, S, B, top_k in CASES:
    agent = make_agent(K, dev, max_batch=B)
    zs = [oracle_z(k, B) for k in range(K)]
    z = torch.stack(zs).to(dev).contiguous()
    rng = np.random.default_rng(1000 + 10 * K + S)
    noise = torch.from_numpy(rng.standard_normal((B, K, S, 4, 2)).astype(np.float32)).to(dev)
    goal = torch.from_numpy((rng.normal(size=(B, 3, 2)) * 4 + np.array([12.0, 0.0])).astype(np.float32)).to(dev)
    target = torch.from_numpy(np.cumsum(np.abs(rng.normal(size=(B, 4, 2))) * 1.5, axis=1).astype(np.float32)).to(dev)
    res = predict(agent, z, S, top_k, noise=noise, target=target)
    assert res["rc"] == 0
    out[(K, S, B, top_k)] = dict(agent=agent, zs=zs, z=z, noise=noise, goal=goal, target=target, res=res)
  return out


def test_sample_normal_known_answers_and_restatement(dev):
  """`rip_sample_normal` gives the normals the known words imply, and 4096 ids from 2^32 - 7 on (the id's high word
  changes inside the launch) agree with `philox_normal` within 1e-5 (derived in the module docstring, not measured).
  Measured on the MI355X: max|d| = 4.77e-7 over the 4096 x 8 values (max|x| 4.02), 1.8e-7 on the two known vectors."""
  for g, want in KNOWN_NORMALS.items():
    got = sample_normal(2024, g, 1, dev)
    print("rip_sample_normal id %d: max|d| to the known answer %.3g" % (g, np.abs(got[0] - want).max()))
    np.testing.assert_allclose(got[0], want, rtol=0, atol=1e-5)
  first, n = 2**32 - 7, 4096
  got, want = sample_normal(2024, first, n, dev), prediction.philox_normal(2024, first, n)
  print("rip_sample_normal against philox_normal: max|d| = %.3g, max|x| = %.3f" % (np.abs(got - want).max(), np.abs(got).max()))
  assert np.isfinite(got).all() and np.abs(got).max() <= 5.77
  np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
  np.testing.assert_array_equal(got[7 + 5], sample_normal(2024, 2**32 + 5, 1, dev)[0])  # any window, the same bits
  np.testing.assert_array_equal(got[100:103], sample_normal(2024, first + 100, 3, dev))
  assert not np.array_equal(sample_normal(2024 + 2**32, 0, 1, dev), sample_normal(2024, 0, 1, dev))  # the key's high word
  # an odd count leaves the rest of the buffer alone
  from oatomobile_amd import _lib
  buf = torch.full((5, 8), SENTINEL, device=dev)
  with torch.cuda.device(dev):
    _lib.check(_lib.load().rip_sample_normal(7, 0, 3, _lib.ptr(buf), _lib.current_stream(dev)))
  assert (buf[3:] == SENTINEL).all() and (buf[:3] != SENTINEL).all()


@pytest.mark.parametrize("K,S,B,top_k", CASES)
def test_candidates_and_scores_with_given_noise(cases, K, S, B, top_k):
  """y_all = the oracle's flow of member j on the given latents (atol 1e-4); q = the oracle's scores of those
  trajectories (rtol 2e-5, atol 2e-3) and the bits of `rip_plan_stats` on the returned y_all.
  Measured on the MI355X: max|dy| 9.5e-7 (y in [-5.7, 5.0]); max|dq| 7.6e-6 at q in [-24.8, -4.2], 0.3 % of the bound."""
  from oracle import reference_cpu as O
  c = cases[(K, S, B, top_k)]
  res, M = c["res"], K * S
  y = res["y_all"].cpu().numpy()
  noise = c["noise"].cpu()
  with torch.no_grad():
    want = np.stack([O.flow_forward(oracle_model(900 + j), noise[:, j].reshape(B * S, 4, 2), c["zs"][j].repeat_interleave(S, 0))
                     [0].numpy().reshape(B, S, 4, 2) for j in range(K)], axis=1).reshape(B, M, 4, 2)
    ref = O.rip_scores([oracle_model(900 + k) for k in range(K)], [zk.repeat_interleave(M, 0) for zk in c["zs"]],
                       torch.from_numpy(y).reshape(B * M, 4, 2), None).numpy().reshape(K, B, M)
  q = res["q"].cpu().numpy()
  err = np.abs(q - ref)
  print("rip_predict K=%d S=%d B=%d: y in [%.1f, %.1f] max|dy| = %.3g; q in [%.1f, %.1f] max|dq| = %.3g, %.3g of the bound" %
        (K, S, B, want.min(), want.max(), np.abs(y - want).max(), ref.min(), ref.max(), err.max(),
         (err / (ATOL_Q + RTOL_Q * np.abs(ref))).max()))
  np.testing.assert_allclose(y, want, rtol=0, atol=1e-4)
  np.testing.assert_allclose(q, ref, rtol=RTOL_Q, atol=ATOL_Q)
  q2, st2 = plan_stats(c["agent"], c["z"], res["y_all"], B, M)
  assert torch.equal(q2, res["q"]) and torch.equal(st2, res["stats"])


@pytest.mark.parametrize("K,S,B,top_k", CASES)
def test_generated_latents_are_philox_normal(cases, dev, K, S, B, top_k):
  """Without `noise`, member j's inverse of y_all gives back `philox_normal` at ids ((row0 + b) K + j) S + s, to 1e-4;
  the second call's ids end just below 2^32 (B = 1) or cross it.  Measured on the MI355X: max|dx| 7.2e-7."""
  c = cases[(K, S, B, top_k)]
  M = K * S
  for row0 in (3, 2**32 // M - 1):
    res = predict(c["agent"], c["z"], S, top_k, seed=2024, row0=row0)
    assert res["rc"] == 0
    want = prediction.philox_normal(2024, row0 * M, B * M).reshape(B, K, S, 8)
    y = res["y_all"].view(B, K, S, 4, 2)
    worst = 0.0
    for j in range(K):
      x, _, _ = hip_model(900 + j, dev)._inverse(y[:, j].reshape(B * S, 4, 2).contiguous(),
                                                 c["z"][j].repeat_interleave(S, 0).contiguous())
      got = x.cpu().numpy().reshape(B, S, 8)
      worst = max(worst, np.abs(got - want[:, j]).max())
      np.testing.assert_allclose(got, want[:, j], rtol=0, atol=1e-4)
    print("rip_predict K=%d S=%d B=%d row0=%d: max|x - philox_normal| = %.3g" % (K, S, B, row0, worst))
    again = predict(c["agent"], c["z"], S, top_k, seed=2024, row0=row0)
    assert torch.equal(again["y_all"], res["y_all"]) and torch.equal(again["index_top"], res["index_top"])
  other = predict(c["agent"], c["z"], S, top_k, seed=2025, row0=3)
  assert not torch.equal(other["y_all"], predict(c["agent"], c["z"], S, top_k, seed=2024, row0=3)["y_all"])


@pytest.mark.parametrize("K,S,B,top_k", CASES)
def test_loss_ranking_and_metrics(cases, K, S, B, top_k):
  """loss_all from the device's own q (exact for WCM / BCM, rtol 1e-6 for MA), the goal term against the oracle
  (rtol 1e-5, atol 2e-4), the ranking against a stable argsort (exact), the gathered rows (bit for bit) and ade / fde
  against float64 numpy (atol 1e-5), for the three algorithms with and without a goal.
  Measured on the MI355X: goal term max|d| 2.3e-5 at terms in [-301, -3.3] (losses up to 320: half an ulp is 1.5e-5);
  ade / fde max|d| 4.8e-7 at errors in [1.4, 9.3]."""
  from oracle import reference_cpu as O
  c = cases[(K, S, B, top_k)]
  M = K * S
  target = c["target"].cpu().numpy().astype(np.float64)
  for algorithm in ("WCM", "MA", "BCM"):
    plain = None
    for goal in (None, c["goal"]):
      res = c["res"] if (algorithm == "WCM" and goal is None) else \
          predict(c["agent"], c["z"], S, top_k, algorithm=algorithm, noise=c["noise"], goal=goal, target=c["target"])
      assert res["rc"] == 0
      assert torch.equal(res["q"], c["res"]["q"]) and torch.equal(res["y_all"], c["res"]["y_all"])
      q, loss = res["q"].cpu().numpy(), res["loss_all"].cpu().numpy()
      if goal is None:
        plain = loss
        if algorithm == "MA":
          np.testing.assert_allclose(loss, numpy_loss(q, algorithm), rtol=1e-6, atol=0)
        else:
          np.testing.assert_array_equal(loss, numpy_loss(q, algorithm))
      else:
        with torch.no_grad():
          term = O.goal_log_likelihood_rows(res["y_all"].cpu().reshape(B * M, 4, 2), goal.cpu().repeat_interleave(M, 0),
                                            EPS).numpy().reshape(B, M)
        got = plain.astype(np.float64) - loss.astype(np.float64)  # loss = aggregate - goal term
        print("rip_predict K=%d S=%d B=%d %s: goal term in [%.1f, %.1f], max|d| = %.3g" %
              (K, S, B, algorithm, term.min(), term.max(), np.abs(got - term).max()))
        np.testing.assert_allclose(got, term, rtol=1e-5, atol=2e-4)
      index = res["index_top"].cpu().numpy()
      np.testing.assert_array_equal(index, np.argsort(loss, axis=1, kind="stable")[:, :top_k])
      rows = np.arange(B)[:, None]
      np.testing.assert_array_equal(res["loss_top"].cpu().numpy(), loss[rows, index])
      y_top = res["y_top"].cpu().numpy()
      np.testing.assert_array_equal(y_top, res["y_all"].cpu().numpy()[rows, index])
      assert (np.diff(res["loss_top"].cpu().numpy(), axis=1) >= 0).all()
      ade, fde = prediction.displacement_errors(y_top, target)
      d_ade, d_fde = np.abs(res["ade"].cpu().numpy() - ade).max(), np.abs(res["fde"].cpu().numpy() - fde).max()
      print("rip_predict K=%d S=%d B=%d %s: ade in [%.2f, %.2f] max|d ade| = %.3g max|d fde| = %.3g" %
            (K, S, B, algorithm, ade.min(), ade.max(), d_ade, d_fde))
      np.testing.assert_allclose(res["ade"].cpu().numpy(), ade, rtol=0, atol=1e-5)
      np.testing.assert_allclose(res["fde"].cpu().numpy(), fde, rtol=0, atol=1e-5)
      # optional outputs NULL: the same top-k
      lean = predict(c["agent"], c["z"], S, top_k, algorithm=algorithm, noise=c["noise"], goal=goal, want_loss_all=False)
      assert lean["rc"] == 0 and lean["ade"] is None
      for name in ("y_top", "loss_top", "index_top"):
        assert torch.equal(lean[name], res[name]), name


def test_planted_tie_and_nan(cases, dev):
  """Duplicated latents of one member give two candidates with the same bits of loss: the lower index ranks first.  A
  NaN latent gives a NaN loss: it ranks last (top_k = M returns every candidate)."""
  K, S, B = 3, 5, 2
  c = cases[(3, 5, 2, 4)]
  M = K * S
  noise = c["noise"].clone()
  noise[0, 1, 3] = noise[0, 1, 0]   # candidates 5 and 8 of observation 0
  noise[1, 2, 4] = noise[1, 2, 1]   # candidates 11 and 14 of observation 1
  noise[1, 0, 2] = float("nan")     # candidate 2 of observation 1
  noise[0, 2, 0, 1, 0] = float("nan")  # one coordinate of candidate 10 of observation 0
  for algorithm in ("WCM", "MA", "BCM"):
    for goal in (None, c["goal"]):
      res = predict(c["agent"], c["z"], S, M, algorithm=algorithm, noise=noise, goal=goal, target=c["target"])
      assert res["rc"] == 0
      loss, index = res["loss_all"].cpu().numpy(), res["index_top"].cpu().numpy()
      assert loss[0, 5] == loss[0, 8] and loss[1, 11] == loss[1, 14]
      assert np.isnan(loss[1, 2]) and np.isnan(loss[0, 10]) and np.isnan(loss).sum() == 2
      np.testing.assert_array_equal(index, np.argsort(loss, axis=1, kind="stable"))
      for b, (lo, hi), nan in ((0, (5, 8), 10), (1, (11, 14), 2)):
        order = list(index[b])
        assert order.index(hi) == order.index(lo) + 1, (algorithm, b, order)
        assert order[-1] == nan and sorted(order) == list(range(M))
      top = res["loss_top"].cpu().numpy()
      assert np.isnan(top[:, -1]).all() and np.isfinite(top[:, :-1]).all()
      assert np.isnan(res["ade"].cpu().numpy()[:, -1]).all() and np.isfinite(res["ade"].cpu().numpy()[:, :-1]).all()
    # with top_k < M the NaN candidate is never chosen
    res = predict(c["agent"], c["z"], S, M - 1, algorithm=algorithm, noise=noise)
    assert torch.isfinite(res["loss_top"]).all()


def test_batch_independence(dev):
  """One call on 5 observations = a call on rows 0-1 (row0 = 0) and a call on rows 2-4 (row0 = 2) at the same z, bit for
  bit: the samples depend on (seed, row, member, sample) and on nothing else."""
  K, S, B, top_k = 3, 5, 5, 4
  agent = make_agent(K, dev, max_batch=B)
  z = torch.stack([oracle_z(k, B) for k in range(K)]).to(dev).contiguous()
  rng = np.random.default_rng(5)
  goal = torch.from_numpy((rng.normal(size=(B, 2, 2)) * 4 + np.array([12.0, 0.0])).astype(np.float32)).to(dev)
  target = torch.from_numpy(np.cumsum(np.abs(rng.normal(size=(B, 4, 2))), axis=1).astype(np.float32)).to(dev)
  for base in (0, 100):
    whole = predict(agent, z, S, top_k, algorithm="MA", goal=goal, target=target, seed=11, row0=base)
    assert whole["rc"] == 0
    for r0, r1 in ((0, 2), (2, 5)):
      part = predict(agent, z[:, r0:r1].contiguous(), S, top_k, algorithm="MA", goal=goal[r0:r1].contiguous(),
                     target=target[r0:r1].contiguous(), seed=11, row0=base + r0)
      assert part["rc"] == 0
      for name in ("y_all", "stats", "loss_all", "y_top", "loss_top", "index_top", "ade", "fde"):
        assert torch.equal(part[name], whole[name][r0:r1]), (base, r0, name)
      assert torch.equal(part["q"], whole["q"][:, r0:r1])
  # row0 shifts the sample ids: other latents at the same z
  assert not torch.equal(predict(agent, z, S, top_k, seed=11, row0=1)["y_all"], predict(agent, z, S, top_k, seed=11, row0=0)["y_all"])


def test_predict_batch_and_coded(dev):
  """`RIPAgent.predict_batch`: `rip_encode_raw` + `rip_predict` with the agent's algorithm and epsilon; the coded entry
  point gives the same bits; `return_candidates` appends (y_all, q, loss_all)."""
  from oatomobile_amd import Prediction, RIPAgent, _lib
  from tests.test_plan_stats import encode_raw
  K, S, B, top_k = 3, 4, 3, 5
  agent = RIPAgent(None, algorithm="BCM", epsilon=EPS, models=[hip_model(900 + k, dev) for k in range(K)], max_batch=B)
  _, lidar, vec, goal = batch_inputs(B, dev)
  target = torch.from_numpy(np.cumsum(np.ones((B, 4, 2)), axis=1).astype(np.float32)).to(dev)
  pred, y_all, q, loss_all = agent.predict_batch(lidar, vec, num_samples=S, top_k=top_k, goal=goal, target=target, seed=9,
                                                 row0=4, return_candidates=True)
  assert isinstance(pred, Prediction)
  assert pred.y.shape == (B, top_k, 4, 2) and pred.index.dtype == torch.int32 and pred.member.shape == (B, top_k)
  assert y_all.shape == (B, K * S, 4, 2) and q.shape == (K, B, K * S) and loss_all.shape == (B, K * S)
  want = predict(agent, encode_raw(agent, lidar, vec), S, top_k, algorithm="BCM", goal=goal, target=target, seed=9, row0=4)
  for got, name in ((pred.y, "y_top"), (pred.loss, "loss_top"), (pred.index, "index_top"), (pred.ade, "ade"), (pred.fde, "fde"),
                    (y_all, "y_all"), (q, "q"), (loss_all, "loss_all")):
    assert torch.equal(got, want[name]), name
  assert torch.equal(pred.member, pred.index // S) and int(pred.member.max()) < K
  lean = agent.predict_batch(lidar, vec, num_samples=S, top_k=top_k, goal=goal, seed=9, row0=4)
  assert isinstance(lean, Prediction) and lean.ade is None and lean.fde is None and torch.equal(lean.y, pred.y)
  codes, lut = code_bev(lidar)
  coded = agent.predict_batch_coded(codes, lut, vec, num_samples=S, top_k=top_k, goal=goal, target=target, seed=9, row0=4)
  for a, b in zip(coded, pred):
    assert torch.equal(a, b)
  noise = torch.randn(B, K, S, 4, 2, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
  with_noise = agent.predict_batch(lidar, vec, num_samples=S, top_k=top_k, noise=noise)
  want = predict(agent, encode_raw(agent, lidar, vec), S, top_k, algorithm="BCM", noise=noise)
  assert torch.equal(with_noise.y, want["y_top"]) and torch.equal(with_noise.index, want["index_top"])
  assert _lib.load().rip_abi_version() == 4


@pytest.fixture(scope="module")
def packed10(tmp_path_factory, dev):
  """10 datums with targets, packed the way tests/test_train_epoch.py packs its caches."""
  from oatomobile_amd import replay
  from tests.test_train_epoch import write_datums
  root = tmp_path_factory.mktemp("predict")
  files = write_datums(str(root / "d"), 10, seed=8)
  cache = replay.pack_cache(files, str(root / "d_cache"), workers=1, targets=True)
  return cache, replay.DeviceCache(cache, dev)


def test_predict_cache(packed10, dev):
  """`replay.predict_cache` over 10 rows in batches of 3 and of 10 = the hand-composed `predict_batch_coded` calls on the
  same rows (row0 = the batch's first row), bit for bit; the data-set means are the numpy reductions of the rows."""
  from oatomobile_amd import replay
  cache, data = packed10
  n, K, S, top_k, seed = 10, 2, 3, 4, 21
  agent = make_agent(K, dev, max_batch=n)
  lut = torch.from_numpy(cache.lut).to(dev)
  stride = replay.downsample_stride(data.L, 4)
  for batch_size in (3, 10):
    res = replay.predict_cache(agent, data, batch_size, S, top_k, seed=seed)
    for name, dtype in (("ade", np.float32), ("fde", np.float32), ("loss", np.float32), ("member", np.int32)):
      assert res[name].shape == (n, top_k) and res[name].dtype == dtype, name
    for i0 in range(0, n, batch_size):
      rows = slice(i0, min(i0 + batch_size, n))
      codes = torch.from_numpy(np.array(cache.codes[rows])).to(dev)
      vec = torch.from_numpy(np.array(cache.vec[rows])).to(dev)
      target = torch.from_numpy(np.array(cache.future[rows], np.float32)[:, 0::stride].copy()).to(dev)
      p = agent.predict_batch_coded(codes, lut, vec, num_samples=S, top_k=top_k, target=target, seed=seed, row0=i0)
      for name, t in (("ade", p.ade), ("fde", p.fde), ("loss", p.loss), ("member", p.member)):
        np.testing.assert_array_equal(res[name][rows], t.cpu().numpy(), err_msg="%s rows %s batch %d" % (name, rows, batch_size))
    assert np.isfinite(res["ade"]).all() and (res["ade"] > 0).all() and (res["member"] < K).all() and (res["member"] >= 0).all()
    assert (res["fde"].min(1) <= res["fde"][:, 0]).all()
    assert (prediction.min_over_k(res["ade"], top_k) <= prediction.min_over_k(res["ade"], 1)).all()
    for name in ("ade", "fde"):
      assert res["min_%s_1" % name] == res[name][:, 0].astype(np.float64).mean()
      assert res["min_%s_k" % name] == res[name].min(1).astype(np.float64).mean()
      assert res["min_%s_k" % name] <= res["min_%s_1" % name]
    assert (np.diff(res["loss"], axis=1) >= 0).all()
  with pytest.raises(ValueError, match="batch_size"):
    replay.predict_cache(agent, data, 11, S, top_k)
  with pytest.raises(ValueError, match="top_k"):
    replay.predict_cache(agent, data, 3, S, K * S + 1)


def test_argument_errors_launch_nothing(dev):
  """Out-of-range S, M, top_k and wrong dtypes: `ValueError` from the Python surface, RIP_EINVAL with a message from the
  ABI, and the output buffers keep their sentinel (nothing was launched)."""
  from oatomobile_amd import _lib
  K, B = 2, 2
  agent = make_agent(K, dev, max_batch=B)
  _, lidar, vec, goal = batch_inputs(B, dev)
  target = torch.zeros(B, 4, 2, device=dev)
  bad = [dict(num_samples=0), dict(num_samples=-1), dict(num_samples=2.0), dict(num_samples=2049),
         dict(num_samples=40, top_k=65), dict(num_samples=2, top_k=5), dict(num_samples=2, top_k=0),
         dict(num_samples=2, target=target.double()), dict(num_samples=2, goal=goal.double()),
         dict(num_samples=2, noise=torch.zeros(B, K, 2, 4, 2, device=dev, dtype=torch.float64)),
         dict(num_samples=2, noise=torch.zeros(B, K, 3, 4, 2, device=dev)), dict(num_samples=2, target=target[:1]),
         dict(num_samples=2, row0=-1), dict(num_samples=2, seed=-1)]
  for kw in bad:
    with pytest.raises(ValueError):
      agent.predict_batch(lidar, vec, **kw)
  with pytest.raises(ValueError, match="float32"):
    agent.predict_batch(lidar.double(), vec, num_samples=2)
  with pytest.raises(RuntimeError, match="must be a tensor on"):
    agent.predict_batch(lidar, vec, num_samples=2, target=target.cpu())
  codes, lut = code_bev(lidar)
  with pytest.raises(ValueError, match="uint8"):
    agent.predict_batch_coded(lidar, lut, vec, num_samples=2)
  with pytest.raises(ValueError):
    agent.predict_batch_coded(codes, lut, vec, num_samples=0)
  # the ABI: illegal values against sentinel-filled buffers of a legal shape
  lib = _lib.load()
  z = torch.stack([oracle_z(k, B) for k in range(K)]).to(dev).contiguous()
  M = K * 40
  bufs = dict(y_all=torch.full((B, M, 4, 2), SENTINEL, device=dev), q=torch.full((K, B, M), SENTINEL, device=dev),
              stats=torch.full((B, M, 4), SENTINEL, device=dev), y_top=torch.full((B, 64, 4, 2), SENTINEL, device=dev),
              loss_top=torch.full((B, 64), SENTINEL, device=dev))
  index_top = torch.full((B, 64), -7, device=dev, dtype=torch.int32)

  def raw(S, top_k, row0=0):
    return lib.rip_predict(agent._handle.raw, _lib.ptr(z), None, 0, EPS, None, None, 0, row0, B, S, top_k, 0, _lib.ptr(bufs["y_all"]),
                           _lib.ptr(bufs["q"]), _lib.ptr(bufs["stats"]), None, _lib.ptr(bufs["y_top"]), _lib.ptr(bufs["loss_top"]),
                           _lib.ptr(index_top, torch.int32), None, None, _lib.current_stream(dev))

  for args, what in (((0, 1), "S=0"), ((-3, 1), "S=-3"), ((2049, 1), "above 4096"), ((40, 65), "top_k=65"), ((2, 5), "top_k=5"),
                     ((2, 0), "top_k=0"), ((2, 1, -1), "row0")):
    assert raw(*args) == _lib.RIP_EINVAL, what
    assert what in lib.rip_last_error().decode(), (what, lib.rip_last_error())
  torch.cuda.synchronize(dev)
  assert all((t == SENTINEL).all() for t in bufs.values()) and (index_top == -7).all()  # nothing was launched
  null = ctypes.c_void_p(0)
  ok = predict(agent, z, 2, 1)
  assert ok["rc"] == 0 and (ok["y_all"] != SENTINEL).all() and (ok["index_top"] >= 0).all()
  buf = lambda name: _lib.ptr(ok[name])  # noqa: E731
  stream = _lib.current_stream(dev)
  tail = (buf("y_top"), buf("loss_top"), _lib.ptr(ok["index_top"], torch.int32))
  assert lib.rip_predict(null, _lib.ptr(z), None, 0, EPS, None, None, 0, 0, B, 2, 1, 0, buf("y_all"), buf("q"), buf("stats"), None,
                         *tail, None, None, stream) == _lib.RIP_EINVAL
  assert lib.rip_predict(agent._handle.raw, null, None, 0, EPS, None, None, 0, 0, B, 2, 1, 0, buf("y_all"), buf("q"),
                         buf("stats"), None, *tail, None, None, stream) == _lib.RIP_EINVAL
  assert lib.rip_predict(agent._handle.raw, _lib.ptr(z), None, 0, EPS, None, None, 0, 0, B, 2, 1, 7, buf("y_all"), buf("q"),
                         buf("stats"), None, *tail, None, None, stream) == _lib.RIP_EINVAL  # unknown algorithm
  assert lib.rip_predict(agent._handle.raw, _lib.ptr(z), _lib.ptr(goal), 65, EPS, None, None, 0, 0, B, 2, 1, 0, buf("y_all"),
                         buf("q"), buf("stats"), None, *tail, None, None, stream) == _lib.RIP_EINVAL  # G above 64
  assert lib.rip_predict(agent._handle.raw, _lib.ptr(z), None, 0, EPS, None, None, 0, 0, B, 2, 1, 0, buf("y_all"), buf("q"),
                         buf("stats"), None, *tail, buf("loss_top"), None, stream) == _lib.RIP_EINVAL  # ade without a target
  with torch.cuda.device(dev):
    assert lib.rip_sample_normal(1, 0, -1, buf("y_all"), stream) == _lib.RIP_EINVAL
    assert lib.rip_sample_normal(1, 0, 4, null, stream) == _lib.RIP_EINVAL
    assert lib.rip_sample_normal(1, 0, 0, null, stream) == 0
