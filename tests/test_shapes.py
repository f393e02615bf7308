"""GPU tests of the input shapes the rest of the suite does not run: BEV sizes other than 200 x 200 through the transform
kernels (LDS-tiled, generic, coded, gather), goal counts other than 10 through every goal-taking kernel, the agent's
captured pipelines on a second BEV size and goal count, and the replay twin after a weight edit.  Every comparison is
against the CPU oracle or a float64 numpy reference (tests/helpers.py), at the tolerance of the 200 x 200 / G = 10 test
of the same call; every test prints its largest deviation (`pytest -s`), the values measured on the MI355X are in the
docstrings."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import TRANSFORM_CASES, bilinear_swap_ref, synth_observation  # noqa: E402
from tests.test_gpu_parity import TOL, candidate_gate, ctx_tensors, hip_model, oracle_model  # noqa: E402

SENTINEL = -12345.5


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. transform kernels
# ---------------------------------------------------------------------------------------------------------------------
def _tiled(C, H, W, out):
  """The host's choice (encoder.hip:launch_transform): the LDS-tiled kernel while a 32-wide output tile's input patch
  fits 68 rows (max(H, W) <= 208 at out = 100) and C <= 3, else one thread per output."""
  scale = np.float32(max(H, W) - 1) / np.float32(out - 1) if out > 1 else np.float32(0.0)
  return bool(np.float32(scale * np.float32(31.0)) + np.float32(3.0) <= np.float32(68.0)) and 1 <= C <= 3


_TRANSFORM_INPUTS = {}


def _transform_case(H, W, out):
  """Dense inputs [3,4,H,W] in [0, 1) (the sparse BEV recipe hides errors behind zeros) and their float64 reference,
  computed once per shape."""
  key = (H, W, out)
  if key not in _TRANSFORM_INPUTS:
    x = np.random.default_rng(4100 + TRANSFORM_CASES.index(key)).random((3, 4, H, W)).astype(np.float32)
    _TRANSFORM_INPUTS[key] = (x, bilinear_swap_ref(x, out))
  return _TRANSFORM_INPUTS[key]


def _quantised(x):
  """256-level codes of x in [0, 1) and their table: lut[codes] is the float32 BEV the coded kernels must reproduce."""
  codes = np.floor(x * 256.0).astype(np.uint8)
  lut = (np.arange(256, dtype=np.float32) / np.float32(256.0)).astype(np.float32)
  return codes, lut


@pytest.mark.parametrize("H,W,out", TRANSFORM_CASES)
def test_transform_shapes_vs_float64_reference(dev, H, W, out):
  """`rip_transform` (B = 3, C = 1..4, both layouts) against tests/helpers.py:bilinear_swap_ref at atol 2e-6 — the suite's
  transform tolerance (test_g1_transform); the blend is four fp32 roundings of values <= 1 — on BEV sizes around the
  tiled kernel's patch bound (208 the last tiled size, 209 the first generic one), non-square and odd sizes, scale 1 (the
  output IS the transposed input, bit for bit), up-sampling (the patch is clipped in every tile), 1-wide inputs, and
  output sizes of one tile, a one-row tile and ragged tiles.  Where both layouts take the tiled kernel the channels-last
  result equals the NCHW result bit for bit.
  Measured on the MI355X: max|d| over the 20 cases — tiled NCHW 1.15e-7, tiled channels-last 1.15e-7, generic (C = 4, or
  max(H, W) > 208 at 100 x 100 outputs) 1.15e-7 in both layouts; 0 at scale 1 and at 1 x 1 / 2 x 2 outputs."""
  from oatomobile_amd import transform_visual
  x, ref = _transform_case(H, W, out)
  assert _tiled(1, 208, 208, 100) and not _tiled(1, 209, 209, 100)
  worst = {}
  for C in (1, 2, 3, 4):
    xc = np.ascontiguousarray(x[:, :C])
    nchw = transform_visual(torch.from_numpy(xc).to(dev), out)
    cl = transform_visual(torch.from_numpy(np.ascontiguousarray(xc.transpose(0, 2, 3, 1))).to(dev), out, channels_last=True)
    assert nchw.shape == cl.shape == (3, C, out, out)
    tiled = _tiled(C, H, W, out)
    for name, got in (("NCHW", nchw.cpu().numpy()), ("channels-last", cl.cpu().numpy())):
      fam = "%s %s" % ("tiled" if tiled else "generic", name)
      worst[fam] = max(worst.get(fam, 0.0), float(np.abs(got - ref[:, :C]).max()))
      np.testing.assert_allclose(got, ref[:, :C], rtol=0, atol=2e-6, err_msg="C=%d %s H=%d W=%d out=%d" % (C, fam, H, W, out))
      if H == out and W == out:
        np.testing.assert_array_equal(got, xc.transpose(0, 1, 3, 2), err_msg="scale 1 must be a transpose (C=%d %s)" % (C, fam))
    if tiled:
      assert torch.equal(cl, nchw), "C=%d H=%d W=%d out=%d: the tiled kernel's two layouts differ" % (C, H, W, out)
  print("rip_transform %d x %d -> %d: max|d| to the float64 reference %s" %
        (H, W, out, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


@pytest.fixture(scope="module")
def coded_models(dev):
  """One fp32 model per BEV channel count 1..3 (`rip_encode_raw_u8` takes C <= 3), three observations per call."""
  return {C: hip_model(40 + C, dev, in_channels=C, max_batch=3) for C in (1, 2, 3)}


def _gather(lib, codes_d, lut_d, rows_d, n, C, H, W, vec_d, fut_d, visual, vec_out, target):
  from oatomobile_amd import _lib
  B = rows_d.shape[0]
  return lib.rip_gather_batch_u8(_lib.ptr(codes_d, torch.uint8), _lib.ptr(lut_d), _lib.ptr(rows_d, torch.int64), B, n, C, H, W, 100,
                                 _lib.ptr(vec_d), _lib.ptr(fut_d), 4, 4, 1, None, _lib.ptr(visual), _lib.ptr(vec_out),
                                 _lib.ptr(target), None, _lib.current_stream(codes_d.device))


@pytest.mark.parametrize("H,W", [(208, 120), (199, 201), (64, 48), (1, 5)])
def test_coded_transform_shapes_bit_identical(dev, coded_models, H, W):
  """The coded transform (uint8 codes + a 256-entry table, looked up while the patch is staged) on BEV sizes other than
  200 x 200: `rip_encode_raw_u8` (fp32 encoder, K = 1, B = 3, C = 1..3) gives the z of `rip_encode_raw` on lut[codes] bit
  for bit, and `rip_gather_batch_u8` (rows [2, 0, 2] of n = 3, C = 1..4) gives `rip_transform(lut[codes[rows]],
  channels_last=1)` bit for bit and the float64 reference at 2e-6.
  Measured on the MI355X: z and the gathered visual bit-identical on the four sizes; gather max|d| to the float64
  reference 1.11e-7.
  Found with this test and fixed: with C = 4 the gather runs the tiled code and `rip_transform` the generic kernel, whose
  blend the compiler had contracted the other way round: 208 x 120 and 64 x 48 differed in the last bit (encoder.hip:
  `bilerp_blend_as_tiled`)."""
  from oatomobile_amd import _lib, transform_visual
  lib = _lib.load()
  x, _ = _transform_case(H, W, 100)
  rng = np.random.default_rng(7)
  vec_np = rng.normal(0, 2, size=(3, 5)).astype(np.float32)
  fut_np = rng.normal(size=(3, 4, 2)).astype(np.float32)
  vec, fut = torch.from_numpy(vec_np).to(dev), torch.from_numpy(fut_np).to(dev)
  rows = [2, 0, 2]
  rows_d = torch.tensor(rows, dtype=torch.int64, device=dev)
  worst = 0.0
  for C in (1, 2, 3, 4):
    codes, lut = _quantised(np.ascontiguousarray(x[:, :C].transpose(0, 2, 3, 1)))  # [3,H,W,C]
    bev = lut[codes]
    codes_d, lut_d, bev_d = torch.from_numpy(codes).to(dev), torch.from_numpy(lut).to(dev), torch.from_numpy(bev).to(dev)
    if C <= 3:
      h = coded_models[C]._handle()
      za, zb = torch.full((1, 3, 64), SENTINEL, device=dev), torch.full((1, 3, 64), SENTINEL, device=dev)
      _lib.check(lib.rip_encode_raw(h.raw, _lib.ptr(bev_d), 1, H, W, _lib.ptr(vec), 3, 0, 1, 0, _lib.ptr(za), h.stream()))
      _lib.check(lib.rip_encode_raw_u8(h.raw, _lib.ptr(codes_d, torch.uint8), _lib.ptr(lut_d), H, W, _lib.ptr(vec), 3, 0, 1, 0,
                                       _lib.ptr(zb), h.stream()))
      assert not (za == SENTINEL).any() and torch.isfinite(za).all()
      assert torch.equal(za, zb), "C=%d H=%d W=%d: z of the coded BEV differs from z of lut[codes]" % (C, H, W)
    visual = torch.full((3, C, 100, 100), SENTINEL, device=dev)
    vec_out, target = torch.full((3, 5), SENTINEL, device=dev), torch.full((3, 4, 2), SENTINEL, device=dev)
    _lib.check(_gather(lib, codes_d, lut_d, rows_d, 3, C, H, W, vec, fut, visual, vec_out, target))
    want = transform_visual(bev_d[rows].contiguous(), 100, channels_last=True)
    assert torch.equal(visual, want), "C=%d H=%d W=%d: the gathered visual differs from rip_transform" % (C, H, W)
    ref = bilinear_swap_ref(bev[rows].transpose(0, 3, 1, 2), 100)
    worst = max(worst, float(np.abs(visual.cpu().numpy() - ref).max()))
    np.testing.assert_allclose(visual.cpu().numpy(), ref, rtol=0, atol=2e-6, err_msg="gather C=%d H=%d W=%d" % (C, H, W))
    np.testing.assert_array_equal(vec_out.cpu().numpy(), vec_np[rows])
    np.testing.assert_array_equal(target.cpu().numpy(), fut_np[rows])
  print("coded transform %d x %d: z and the gathered visual bit-identical; gather max|d| to the float64 reference %.3g" % (H, W, worst))


@pytest.mark.parametrize("H,W", [(209, 209), (400, 100)])
def test_coded_transform_refuses_more_than_a_factor_of_two(dev, coded_models, H, W):
  """A coded BEV is the tiled kernel's only: a down-sampling factor beyond 2 (209 x 209, 400 x 100 -> 100) is RIP_EINVAL
  from `rip_encode_raw_u8` and `rip_gather_batch_u8`, and nothing is written."""
  from oatomobile_amd import _lib
  lib = _lib.load()
  lut_d = torch.from_numpy(_quantised(np.zeros(1))[1]).to(dev)
  vec, fut = torch.zeros(3, 5, device=dev), torch.zeros(3, 4, 2, device=dev)
  rows_d = torch.tensor([2, 0, 2], dtype=torch.int64, device=dev)
  for C in (1, 2, 3, 4):
    codes_d = torch.zeros((3, H, W, C), dtype=torch.uint8, device=dev)
    if C <= 3:
      h = coded_models[C]._handle()
      z = torch.full((1, 3, 64), SENTINEL, device=dev)
      rc = lib.rip_encode_raw_u8(h.raw, _lib.ptr(codes_d, torch.uint8), _lib.ptr(lut_d), H, W, _lib.ptr(vec), 3, 0, 1, 0, _lib.ptr(z),
                                 h.stream())
      assert rc == _lib.RIP_EINVAL and b"not supported" in lib.rip_last_error()
      torch.cuda.synchronize(dev)
      assert (z == SENTINEL).all()
    visual = torch.full((3, C, 100, 100), SENTINEL, device=dev)
    vec_out, target = torch.full((3, 5), SENTINEL, device=dev), torch.full((3, 4, 2), SENTINEL, device=dev)
    rc = _gather(lib, codes_d, lut_d, rows_d, 3, C, H, W, vec, fut, visual, vec_out, target)
    assert rc == _lib.RIP_EINVAL and b"not supported" in lib.rip_last_error()
    torch.cuda.synchronize(dev)
    assert (visual == SENTINEL).all() and (vec_out == SENTINEL).all() and (target == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. goal counts
# ---------------------------------------------------------------------------------------------------------------------
GK, GB, GN = 3, 3, 16  # models, observations, candidates of the goal-count tests


def _goals(rng, rows, G):
  """`rows` goals by the recipe of tests/helpers.py:synth_observation, each row its own draw: ~100 m away at G = 64, where
  one waypoint dominates the mixture and the others underflow (what the two-pass maximum of `goal_ll` is there for)."""
  return np.stack([np.cumsum(np.abs(rng.normal(size=(G, 2))) * 2.0, axis=0) for _ in range(rows)]).astype(np.float32)


@pytest.fixture(scope="module")
def goal_models(dev):
  """Three models (HIP and oracle, seeds 300..302), one agent per search kernel built on first use, and per goal count the
  inputs and the oracle's teacher-forced step — computed once, shared by the four kernels."""
  from oatomobile_amd import RIPAgent
  from oracle import reference_cpu as O
  hips = [hip_model(300 + k, dev) for k in range(GK)]
  refs = [oracle_model(300 + k) for k in range(GK)]
  agents, cases = {}, {}

  def agent(kernel):
    if kernel not in agents:
      agents[kernel] = RIPAgent(None, algorithm="MA", models=hips, num_candidates=GN, seed=9, search_kernel=kernel, max_batch=GB)
    return agents[kernel]

  def case(G):
    if G not in cases:
      rng = np.random.default_rng(5000 + G)
      z = np.abs(rng.normal(size=(GK, GB, 64))).astype(np.float32)  # a ReLU output; every (model, observation) its own row
      z[:, :, ::7] = 0.0
      goal = _goals(rng, GB, G)
      x = rng.normal(size=(GB, GN, 4, 2)).astype(np.float32)
      post, loss, grad = [], [], []
      for b in range(GB):
        res = O.rip_search(refs, [torch.from_numpy(z[k, b:b + 1]) for k in range(GK)], torch.from_numpy(goal[b:b + 1]),
                           torch.from_numpy(x[b]), algorithm="MA", num_steps=1)
        post.append(res["trace_post"].numpy()[0])
        loss.append(res["trace_loss"].numpy()[0])
        grad.append(res["trace_grad"].numpy()[0])
      cases[G] = dict(z=z, goal=goal, x=x, post=np.stack(post), loss=np.stack(loss), grad=np.stack(grad))  # [B,K,N] [B,N] [B,N,4,2]
    return cases[G]

  return dict(hips=hips, refs=refs, agent=agent, case=case)


@pytest.mark.parametrize("G", [1, 3, 20, 64])
@pytest.mark.parametrize("kernel", ["chain", "phase", "split", "pair"])
def test_teacher_forced_step_goal_counts(dev, goal_models, kernel, G):
  """One teacher-forced Adam step of `rip_search` (K = 3, algorithm MA: every member's adjoint reaches the gradient; N = 16)
  on B = 3 observations with DIFFERENT z rows and DIFFERENT goals of G = 1 / 3 / 20 / 64 waypoints, each observation against
  the oracle's step: posteriors and loss at rtol 1e-5 + atol 1e-4, gradients at rtol 1e-4 + atol 1e-4, the bars of
  test_teacher_forced_steps_vs_oracle, every candidate.  A goal row stride, an LDS staging loop or a log G term that only
  holds at G = 10 fails here.
  Measured on the MI355X at G = 64, max |d post| / |d grad|: chain 5.7e-6 / 2.4e-6, phase 5.7e-6 / 1.9e-6, split 5.7e-6 /
  1.9e-6, pair 5.7e-6 / 1.9e-6 (posteriors in [-34.9, -12.7], max |grad| 8.4); over all 16 cases 7.6e-6 / 5.3e-6."""
  from oatomobile_amd import _lib
  c, agent = goal_models["case"](G), goal_models["agent"](kernel)
  z, goal, x = (torch.from_numpy(c[k]).to(dev) for k in ("z", "goal", "x"))
  nan = float("nan")
  lb, tp, tg = torch.full((GB, GN), nan, device=dev), torch.full((1, GK, GB, GN), nan, device=dev), torch.full((1, GB, GN, 4, 2), nan, device=dev)
  h = agent._handle
  _lib.check(_lib.load().rip_search(h.raw, _lib.ptr(z), _lib.ptr(goal), _lib.ptr(x), GB, GN, G, _lib.ALGORITHMS["MA"], 1, 0.1, 1.0,
                                    None, None, _lib.ptr(lb), None, _lib.ptr(tp), None, _lib.ptr(tg), h.stream()))
  post_h, loss_h, grad_h = tp.cpu().numpy()[0].transpose(1, 0, 2), lb.cpu().numpy(), tg.cpu().numpy()[0]
  print("%s G=%d teacher-forced: max |d post| %.3g (posteriors in [%.4g, %.4g]), max |d loss| %.3g, max |d grad| %.3g (max |grad| %.3g)" %
        (kernel, G, np.abs(post_h - c["post"]).max(), c["post"].min(), c["post"].max(),
         np.abs(loss_h - np.minimum(c["loss"], 1000.0)).max(), np.abs(grad_h - c["grad"]).max(), np.abs(c["grad"]).max()))
  np.testing.assert_allclose(post_h, c["post"], rtol=1e-5, atol=TOL)
  np.testing.assert_allclose(loss_h, np.minimum(c["loss"], 1000.0), rtol=1e-5, atol=TOL)
  np.testing.assert_allclose(grad_h, c["grad"], rtol=1e-4, atol=TOL)


@pytest.mark.parametrize("G", [20, 64])
def test_score_goal_rows_dim_forward_and_predict_goal_counts(dev, goal_models, G):
  """One call each at G = 20 (the reference's observation spec) and G = 64 (the ABI's limit), B = 3 with a goal of its own
  per row, against the oracle: `rip_score` with a goal (rtol 2e-5 + atol 2e-3, test_g8_scores), `rip_goal_likelihood` at
  goal_rows = N and 1, eps 0.5 and 1 (rtol 1e-5 + atol 2e-4, test_g4_goal), `ImitativeModel.forward(num_steps=20)` (atol
  1e-4, test_g7_dim_forward) and the goal term of `rip_predict` (rtol 1e-5 + atol 2e-4, test_loss_ranking_and_metrics).
  Measured on the MI355X (G = 20 / 64): `rip_score` max|d| 4.6e-5 / 4.6e-5 at scores down to -258 / -362; goal rows 1.9e-6 /
  9.5e-7 at rows down to -377 / -304; `forward` max|dy| 1.8e-6 / 1.1e-6; `rip_predict` goal term 3.8e-6 / 9.5e-7."""
  from oatomobile_amd import _lib
  from oracle import reference_cpu as O
  lib, hips, refs = _lib.load(), goal_models["hips"], goal_models["refs"]
  agent = goal_models["agent"]("chain")
  h = agent._handle
  rng = np.random.default_rng(6000 + G)
  z_np = np.abs(rng.normal(size=(GK, GB, 64))).astype(np.float32)
  goal_np = _goals(rng, GB, G)
  y_np = np.cumsum(np.abs(rng.normal(size=(GB, GN, 4, 2))) * 3.0, axis=2).astype(np.float32)  # plausible plans: forward, metres apart
  z, goal, y = (torch.from_numpy(a).to(dev) for a in (z_np, goal_np, y_np))
  # rip_score
  S = torch.full((GK, GB, GN), float("nan"), device=dev)
  _lib.check(lib.rip_score(h.raw, 0, GK, _lib.ptr(z), _lib.ptr(y), _lib.ptr(goal), GB, GN, G, 1.0, _lib.ptr(S), h.stream()))
  with torch.no_grad():
    S_o = np.stack([O.rip_scores(refs, [torch.from_numpy(z_np[k, b:b + 1]) for k in range(GK)], torch.from_numpy(y_np[b]),
                                 torch.from_numpy(goal_np[b:b + 1])).numpy() for b in range(GB)], axis=1)  # [K,B,N]
  print("G=%d rip_score: max|d| = %.3g at scores in [%.4g, %.4g]" % (G, np.abs(S.cpu().numpy() - S_o).max(), S_o.min(), S_o.max()))
  np.testing.assert_allclose(S.cpu().numpy(), S_o, rtol=2e-5, atol=2e-3)
  # rip_goal_likelihood: a goal per row, and one goal for all rows
  rows_y = torch.from_numpy(y_np.reshape(GB * GN, 4, 2))
  rows_goal = torch.from_numpy(_goals(rng, GB * GN, G))
  for eps in (0.5, 1.0):
    for g in (rows_goal, rows_goal[5:6]):
      got = hips[0]._goal_likelihood_rows(rows_y.to(dev), g.to(dev), epsilon=eps).cpu().numpy()
      want = O.goal_log_likelihood_rows(rows_y, g, eps).numpy()
      print("G=%d rip_goal_likelihood goal_rows=%d eps=%g: max|d| = %.3g at rows in [%.4g, %.4g]" %
            (G, g.shape[0], eps, np.abs(got - want).max(), want.min(), want.max()))
      np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-4)
  # ImitativeModel.forward: the whole-batch mode search of one model
  obs = [synth_observation(np.random.default_rng(7000 + G + 10 * b), G=G) for b in range(GB)]
  ctx = ctx_tensors(obs, dev)
  goal_obs = torch.stack([torch.from_numpy(o["goal"][:, :2].copy()) for o in obs])
  x0 = torch.from_numpy(np.repeat(rng.normal(size=(1, 4, 2)).astype(np.float32), GB, axis=0))  # dim/model.py:100-104: one sample, repeated
  yh = hips[0](num_steps=20, goal=goal_obs.to(dev), lr=5e-2, epsilon=1.0, x0=x0, **ctx).cpu().numpy()
  with torch.no_grad():
    zo = O.params(refs[0], **{k: v.cpu() for k, v in ctx.items()})
  yo, _ = O.dim_forward(refs[0], zo, x0, 20, goal=goal_obs, lr=5e-2, epsilon=1.0)
  print("G=%d ImitativeModel.forward(num_steps=20): max|dy| = %.3g" % (G, np.abs(yh - yo.numpy()).max()))
  np.testing.assert_allclose(yh, yo.numpy(), atol=TOL)
  # rip_predict: the goal term = loss without a goal - loss with it
  Sn = 4
  noise = torch.from_numpy(rng.standard_normal((GB, GK, Sn, 4, 2)).astype(np.float32)).to(dev)
  plain = agent._predict(z, GB, Sn, 1, None, None, noise, 0, 0, True)
  withg = agent._predict(z, GB, Sn, 1, goal, None, noise, 0, 0, True)
  assert torch.equal(plain[1], withg[1])
  y_all = withg[1].cpu()
  M = GK * Sn
  term = O.goal_log_likelihood_rows(y_all.reshape(GB * M, 4, 2), torch.from_numpy(goal_np).repeat_interleave(M, 0), 1.0).numpy().reshape(GB, M)
  got = plain[3].cpu().numpy().astype(np.float64) - withg[3].cpu().numpy().astype(np.float64)
  print("G=%d rip_predict: goal term in [%.4g, %.4g], max|d| = %.3g" % (G, term.min(), term.max(), np.abs(got - term).max()))
  np.testing.assert_allclose(got, term, rtol=1e-5, atol=2e-4)


def test_goal_count_65_is_refused_before_any_launch(dev, goal_models):
  """G = 65 is one past the ABI's limit (RIP_MAX_GOALS = 64: the chain kernels stage 2 x 64 floats of goal in LDS):
  `plan_batch` raises `RipError`, `rip_score` and `rip_predict` return RIP_EINVAL, the sentinel-filled outputs stay
  untouched and the kernel log shows that `plan_batch` did not launch its encoder either.
  Found with this test and fixed: `rip_score` took any G >= 1, and `rip_act` / `rip_act_stats` checked G only after the
  transform and the K encoders had been launched."""
  from oatomobile_amd import _lib
  lib, agent = _lib.load(), goal_models["agent"]("chain")
  h = agent._handle
  G = 65
  rng = np.random.default_rng(65)
  goal = torch.from_numpy(_goals(rng, GB, G)).to(dev)
  z = torch.from_numpy(np.abs(rng.normal(size=(GK, GB, 64))).astype(np.float32)).to(dev)
  y = torch.from_numpy(rng.normal(size=(GB, GN, 4, 2)).astype(np.float32)).to(dev)
  lidar, vec = torch.zeros(GB, 200, 200, 2, device=dev), torch.zeros(GB, 5, device=dev)
  h.set_option(_lib.OPT_KERNEL_LOG, 1)  # (clears the log)
  try:
    for kw in (dict(), dict(return_stats=True)):
      out = torch.full((GB, 4, 2), SENTINEL, device=dev)
      with pytest.raises(_lib.RipError, match=r"G=65 must be in \[1,64\]"):
        agent.plan_batch(lidar, vec, goal, out=out, **kw)
      torch.cuda.synchronize(dev)
      assert (out == SENTINEL).all() and h.kernel_log() == []
    agent.plan_batch(lidar, vec, goal[:, :64].contiguous())  # the limit itself runs, and the log does record launches
    assert h.kernel_log() != []
  finally:
    h.set_option(_lib.OPT_KERNEL_LOG, 0)
  S = torch.full((GK, GB, GN), SENTINEL, device=dev)
  rc = lib.rip_score(h.raw, 0, GK, _lib.ptr(z), _lib.ptr(y), _lib.ptr(goal), GB, GN, G, 1.0, _lib.ptr(S), h.stream())
  assert rc == _lib.RIP_EINVAL and b"G=65" in lib.rip_last_error()
  outs = [torch.full(s, SENTINEL, device=dev) for s in ((GB, GK, 4, 2), (GK, GB, GK), (GB, GK, 4), (GB, GK), (GB, 1, 4, 2), (GB, 1))]
  index = torch.full((GB, 1), -7, device=dev, dtype=torch.int32)
  rc = lib.rip_predict(h.raw, _lib.ptr(z), _lib.ptr(goal), G, 1.0, None, None, 0, 0, GB, 1, 1, 0, _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                       _lib.ptr(outs[2]), _lib.ptr(outs[3]), _lib.ptr(outs[4]), _lib.ptr(outs[5]), _lib.ptr(index, torch.int32), None,
                       None, h.stream())
  assert rc == _lib.RIP_EINVAL and b"G=65" in lib.rip_last_error()
  torch.cuda.synchronize(dev)
  assert (S == SENTINEL).all() and all((o == SENTINEL).all() for o in outs) and (index == -7).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the agent on another BEV size and goal count
# ---------------------------------------------------------------------------------------------------------------------
def test_agent_pipelines_per_bev_size_and_goal_count(dev):
  """`RIPAgent.__call__` keys its captured one-observation pipelines on (H, W, G).  ONE agent (K = 2, MA, N = 8, fp32
  encoder, graph=True) is called with A: 200 x 200 / G = 10, B: 120 x 208 / G = 20 (the tiled transform, non-square),
  C: 160 x 240 / G = 3 (the generic transform), then A and B again: three pipelines, the second visit returns the bits
  of the first, every result equals an eager (graph=False) agent's bit for bit and passes the candidate gate of
  test_search_candidates_vs_oracle against `O.rip_call` with no outlier allowed.  `plan_batch` on three 120 x 208 / G = 20
  observations equals the three single calls within 1e-5 (test_batched_act_matches_single).
  Measured on the MI355X: no candidate outside the gate (max |d loss| 4.8e-6), winner plans within 1.1e-6 m of the oracle's;
  three captured hipGraphs; `plan_batch` against the single calls max|d| 0."""
  from oatomobile_amd import RIPAgent
  from oatomobile_amd.agents import interpolate_plan
  from oracle import reference_cpu as O
  K, N = 2, 8
  models = [hip_model(820 + k, dev) for k in range(K)]
  refs = [oracle_model(820 + k) for k in range(K)]
  g_agent = RIPAgent(None, algorithm="MA", models=models, num_candidates=N, seed=3, graph=True, max_batch=3)
  e_agent = RIPAgent(None, algorithm="MA", models=models, num_candidates=N, seed=3, graph=False, max_batch=3)
  obs = dict(A=synth_observation(np.random.default_rng(8100), G=10),
             B=synth_observation(np.random.default_rng(8101), G=20, H=120, W=208),
             C=synth_observation(np.random.default_rng(8102), G=3, H=160, W=240))
  first = {}
  for visit, name in enumerate("ABCAB"):
    ob = obs[name]
    out = g_agent(dict(ob))
    assert out.shape == (30, 3)
    if name in first:
      np.testing.assert_array_equal(out, first[name], err_msg="second visit to observation %s" % name)
      continue
    first[name] = out
    np.testing.assert_array_equal(out, e_agent(dict(ob)), err_msg="graph vs eager, observation %s" % name)
    lidar = torch.from_numpy(ob["lidar"]).to(dev)[None]
    vec = torch.tensor([[*ob["velocity"], ob["is_at_traffic_light"], ob["traffic_light_state"]]], device=dev)
    goal = torch.from_numpy(ob["goal"][None, :, :2].copy()).to(dev)
    plan, loss = e_agent.plan_batch(lidar, vec, goal, return_loss=True)
    np.testing.assert_array_equal(out, interpolate_plan(plan.cpu().numpy()[0]))
    _, res = O.rip_call(refs, ob["lidar"], ob["velocity"], ob["is_at_traffic_light"], ob["traffic_light_state"], ob["goal"],
                        x0=g_agent._x0_rows.cpu(), algorithm="MA")
    candidate_gate("agent %s %dx%d G=%d" % ((name,) + ob["lidar"].shape[:2] + (ob["goal"].shape[0],)), loss.cpu().numpy()[0],
                   res["loss_best"].numpy(), plan.cpu().numpy()[0], res["plan"].numpy(), ceiling=0)
  assert sorted(g_agent._online) == [(120, 208, 20), (160, 240, 3), (200, 200, 10)]
  print("online pipelines: %s, hipGraph captured = %s" % (sorted(g_agent._online), [st["graph"] is not None for st in g_agent._online.values()]))
  # plan_batch on three observations of the second size
  batch = [synth_observation(np.random.default_rng(8110 + i), G=20, H=120, W=208) for i in range(3)]
  lidar = torch.stack([torch.from_numpy(o["lidar"]) for o in batch]).to(dev)
  vec = torch.tensor([[*o["velocity"], o["is_at_traffic_light"], o["traffic_light_state"]] for o in batch], device=dev)
  goal = torch.stack([torch.from_numpy(o["goal"][:, :2].copy()) for o in batch]).to(dev)
  plans = g_agent.plan_batch(lidar, vec, goal, interpolate=True).cpu().numpy()
  singles = np.stack([g_agent(dict(o)) for o in batch])
  print("plan_batch 3 x (120 x 208, G = 20) vs single calls: max|d| = %.3g" % np.abs(plans - singles).max())
  np.testing.assert_allclose(plans, singles, rtol=0, atol=1e-5)
  assert len(g_agent._online) == 3


# ---------------------------------------------------------------------------------------------------------------------
# 5. the replay twin
# ---------------------------------------------------------------------------------------------------------------------
def test_replay_twin_follows_weight_edits_and_handle_options(dev, tmp_path):
  """`replay_cache(streams=2)` plans its odd batches on a cached second handle (`RIPAgent.replay_twin`).  Over a 10-row
  cache in batches of 3: two streams equal one stream bit for bit (a) as built, (b) after an in-place edit of a flow
  weight of model 0 followed by `agent.refresh()` — and the plans differ from (a) —, (c) after another edit followed by
  `model.refresh()`, (d) with `OPT_ENCODER_VARIANT = ENC_VAR_FP32_LAYERWISE` set on the agent's handle after construction.
  Found by reading the code and fixed with this test: the twin kept its weight snapshot through `agent.refresh()` (its
  model versions still matched, so every odd batch was planned with the old weights), and options set on the agent's
  handle after construction never reached the twin's."""
  from oatomobile_amd import RIPAgent, _lib, replay
  models = [hip_model(830 + k, dev) for k in range(2)]
  agent = RIPAgent(None, algorithm="MA", models=models, num_candidates=8, max_batch=3, seed=4)
  ep = replay.Episode(str(tmp_path), "ep")
  rng = np.random.default_rng(5)
  for i in range(10):
    o = synth_observation(np.random.default_rng(8300 + i))
    fut = np.cumsum(np.abs(rng.normal(size=(80, 3))) * 0.4, axis=0).astype(np.float32)
    ep.append("f%02d" % i, lidar=o["lidar"], velocity=o["velocity"], is_at_traffic_light=o["is_at_traffic_light"],
              traffic_light_state=o["traffic_light_state"], player_future=fut)
  cache = replay.pack_cache(ep.files(), str(tmp_path / "cache"))

  def both(what):
    one, two = replay.replay_cache(agent, cache, 3), replay.replay_cache(agent, cache, 3, streams=2)
    assert one.shape == (10, 4, 2) and np.isfinite(one).all()
    odd = np.r_[3:6, 9:10]  # the rows of the odd batches: the twin's
    print("replay twin, %s: max|d| two streams vs one = %.3g (rows of the twin's batches: %.3g)" %
          (what, np.abs(two - one).max(), np.abs(two[odd] - one[odd]).max()))
    np.testing.assert_array_equal(two, one, err_msg="streams=2 differs from streams=1 %s" % what)
    return one

  built = both("as built")
  weight = models[0].get_parameter("_decoder._decoder.weight_hh")
  with torch.no_grad():
    weight.mul_(1.25)
  agent.refresh()
  edited = both("after an in-place weight edit and agent.refresh()")
  assert np.abs(edited - built).max() > 1e-4, "the edit did not change the plans"
  with torch.no_grad():
    weight.mul_(0.5)
  models[0].refresh()
  again = both("after an in-place weight edit and model.refresh()")
  assert np.abs(again - edited).max() > 1e-4
  agent._handle.set_option(_lib.OPT_ENCODER_VARIANT, _lib.ENC_VAR_FP32_LAYERWISE)
  both("with the layer-wise fp32 encoder selected after construction")
  assert agent._replay_twin._handle.options[_lib.OPT_ENCODER_VARIANT] == _lib.ENC_VAR_FP32_LAYERWISE
