"""Autograd through `_forward` / `_inverse` / `_goal_likelihood` (HIP VJP kernels: rip_flow_vjp, rip_goal_likelihood_vjp).

The reference's planners (rip/agent.py:85-137, dim/model.py:100-139) are autograd programs over these methods; here
they run on this package's models and are checked against the oracle's own autograd (float64) and the g6 / g7 goldens.

Worst errors measured on the MI355X (max over elements of |d_hip - d_ref| / max(1, max|d_ref|), bound 1e-4):
  forward VJP 7.9e-7, inverse VJP 5.5e-7, inverse VJP on g2's large-|y| rows (y2) 3.9e-7 (dx / dy / dz alike);
  goal VJP max|d_hip - d_ref| 6.3e-5 absolute (bound: rtol 1e-5, atol 2e-4, as g4).
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oatomobile_amd import weights as W  # noqa: E402
from tests.helpers import synth_observation  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
WORST = {}


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def hip_model(seed, dev):
  from oatomobile_amd import ImitativeModel
  return ImitativeModel.synthetic(seed).to(dev)


def oracle64(seed):
  from oracle import reference_cpu as O
  return O.OracleImitativeModel.from_numpy_state_dict(W.synthetic_state_dict(seed)).double()


def _rows(g, n, key, rng, noise):
  """n rows built from g2's 128: the fixture itself for n <= 128, beyond that its rows again with a small perturbation."""
  a = g[key]
  if n <= a.shape[0]:
    return np.ascontiguousarray(a[:n])
  idx = np.arange(n) % a.shape[0]
  return (a[idx] + noise * rng.standard_normal(a[idx].shape)).astype(np.float32)


def _ref_vjp(m64, mode, inp, z, z_rows, cots):
  """float64 oracle: (d inp, d z) of sum_i <out_i, cot_i> (cot None = zero)."""
  from oracle import reference_cpu as O
  a = torch.tensor(inp, dtype=torch.float64, requires_grad=True)
  z0 = torch.tensor(z, dtype=torch.float64, requires_grad=True)
  zz = z0.expand(a.shape[0], -1) if z_rows == 1 else z0
  outs = O.flow_forward(m64, a, zz) if mode == 0 else O.flow_inverse(m64, a, zz)
  loss = sum((o * torch.tensor(c, dtype=torch.float64)).sum() for o, c in zip(outs, cots) if c is not None)
  da, dz = torch.autograd.grad(loss, [a, z0])
  return da.numpy(), dz.numpy()


def _hip_vjp(m, mode, inp, z, cots, dev, want_in=True, want_z=True):
  a = torch.tensor(inp, device=dev, requires_grad=want_in)
  zt = torch.tensor(z, device=dev, requires_grad=want_z)
  outs = m._forward(a, zt) if mode == 0 else m._inverse(a, zt)
  pairs = [(o, torch.tensor(c, device=dev)) for o, c in zip(outs, cots) if c is not None]
  wrt = [t for t in (a, zt) if t.requires_grad]
  grads = list(torch.autograd.grad([o for o, _ in pairs], wrt, [c for _, c in pairs]))
  return (grads.pop(0) if want_in else None), (grads.pop(0) if want_z else None)


def _check(tag, got, want):
  got = got.detach().cpu().numpy()
  assert got.shape == want.shape and got.dtype == np.float32, (tag, got.shape, want.shape, got.dtype)
  scale = max(1.0, float(np.abs(want).max()))
  err = float(np.abs(got.astype(np.float64) - want).max()) / scale
  key = tag.split(" ")[0]
  WORST[key] = max(WORST.get(key, 0.0), err)
  assert err <= TOL, "%s: max|d_hip - d_ref| / max(1, max|d_ref|) = %.3g" % (tag, err)


# cotangent sets per mode: every output, each output alone (the others NULL)
COTS = {0: {"all": (1, 1), "y": (1, 0), "lad": (0, 1)},
        1: {"all": (1, 1, 1), "x": (1, 0, 0), "lp": (0, 1, 0), "lad": (0, 0, 1)}}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 65, 128, 257, 4096])
@pytest.mark.parametrize("bcast", [False, True])
def test_flow_vjp_vs_oracle_float64(golden, dev, mode, n, bcast):
  """Both VJP modes against the oracle's autograd in float64: N in {1, 3, 65, 257, 4096} plus g2's own 128 rows, z per
  row and broadcast ([1,64]), random cotangents on every output and on each output alone, and NULL outputs."""
  g = golden("g2_flow.npz")
  seed = int(g["weight_seed"])
  m, m64 = hip_model(seed, dev), oracle64(seed)
  rng = np.random.default_rng(1000 + n)
  inp = _rows(g, n, "x" if mode == 0 else "y", rng, 0.1)
  z = _rows(g, 1 if bcast else n, "z", rng, 0.05)
  z_rows = 1 if bcast else n
  shapes = [(n, 4, 2), (n,)] if mode == 0 else [(n, 4, 2), (n,), (n,)]
  for name, on in COTS[mode].items():
    cots = [rng.standard_normal(s).astype(np.float32) if o else None for s, o in zip(shapes, on)]
    ref_in, ref_z = _ref_vjp(m64, mode, inp, z, z_rows, cots)
    tag = "mode%d n=%d bcast=%d cot=%s" % (mode, n, bcast, name)
    d_in, dz = _hip_vjp(m, mode, inp, z, cots, dev)
    _check(tag + " d_in", d_in, ref_in)
    _check(tag + " dz", dz, ref_z)
    if name == "all":  # one output not wanted: the kernel gets NULL for it and must still give the other
      d_in, dz = _hip_vjp(m, mode, inp, z, cots, dev, want_z=False)
      assert dz is None
      _check(tag + " d_in-only", d_in, ref_in)
      d_in, dz = _hip_vjp(m, mode, inp, z, cots, dev, want_in=False)
      assert d_in is None
      _check(tag + " dz-only", dz, ref_z)
  print("worst so far:", {k: "%.2g" % v for k, v in WORST.items()})


@pytest.mark.parametrize("bcast", [False, True])
def test_inverse_vjp_large_y_rows(golden, dev, bcast):
  """g2's y2: rows far outside the data (|x| ~ 1e2..1e3, |log_prob| ~ 1e3) through the inverse VJP."""
  g = golden("g2_flow.npz")
  seed = int(g["weight_seed"])
  m, m64 = hip_model(seed, dev), oracle64(seed)
  rng = np.random.default_rng(7)
  y2, z = np.ascontiguousarray(g["y2"]), np.ascontiguousarray(g["z"][:1] if bcast else g["z"])
  n = y2.shape[0]
  for name, on in COTS[1].items():
    cots = [rng.standard_normal(s).astype(np.float32) if o else None for s, o in zip([(n, 4, 2), (n,), (n,)], on)]
    ref_in, ref_z = _ref_vjp(m64, 1, y2, z, 1 if bcast else n, cots)
    d_in, dz = _hip_vjp(m, 1, y2, z, cots, dev)
    _check("y2 bcast=%d cot=%s d_in" % (bcast, name), d_in, ref_in)
    _check("y2 bcast=%d cot=%s dz" % (bcast, name), dz, ref_z)
  print("worst so far:", {k: "%.2g" % v for k, v in WORST.items()})


@pytest.mark.parametrize("eps", [0.5, 1.0])
@pytest.mark.parametrize("goal_rows", ["N", "1"])
def test_goal_vjp_vs_oracle_float64(golden, dev, eps, goal_rows):
  """rip_goal_likelihood_vjp against the oracle's autograd on g4's plans and goals, per row and through the batch mean."""
  from oracle import reference_cpu as O
  g = golden("g4_goal.npz")
  m = hip_model(3, dev)
  y = g["y"]
  goal = g["goal"] if goal_rows == "N" else g["goal"][:1]
  grow = np.random.default_rng(11).standard_normal(y.shape[0]).astype(np.float32)
  y64 = torch.tensor(y, dtype=torch.float64, requires_grad=True)
  rows = O.goal_log_likelihood_rows(y64, torch.tensor(goal, dtype=torch.float64), eps)
  (want,) = torch.autograd.grad((rows * torch.tensor(grow, dtype=torch.float64)).sum(), [y64], retain_graph=True)
  (want_mean,) = torch.autograd.grad(rows.mean(0), [y64])
  yt = torch.tensor(y, device=dev, requires_grad=True)
  gt = torch.tensor(goal, device=dev)
  (got,) = torch.autograd.grad(m._goal_likelihood_rows(yt, gt, epsilon=eps), [yt], [torch.tensor(grow, device=dev)])
  (got_mean,) = torch.autograd.grad(m._goal_likelihood(yt, gt, epsilon=eps), [yt])
  for tag, a, b in (("rows", got, want), ("mean", got_mean, want_mean)):
    a = a.cpu().numpy()
    err = float(np.abs(a - b.numpy()).max())
    WORST["goal"] = max(WORST.get("goal", 0.0), err)
    np.testing.assert_allclose(a, b.numpy(), rtol=1e-5, atol=2e-4, err_msg=tag)
    assert np.all(a[:, :3] == 0.0), "only the last waypoint carries a goal gradient"
  print("goal vjp eps=%g goal_rows=%s: max|err| = %.3g" % (eps, goal_rows, WORST["goal"]))


def _aggregate(neg_post, algo):
  if algo == "WCM":
    return torch.min(neg_post, dim=0)[0]
  if algo == "BCM":
    return torch.max(neg_post, dim=0)[0]
  return torch.mean(neg_post, dim=0)


@pytest.mark.parametrize("algo", ["WCM", "MA", "BCM"])
def test_reference_rip_recipe_through_autograd(golden, dev, algo):
  """The RIPAgent.__call__ loop (rip/agent.py:85-137) restated as a user would write it against this package's
  methods: torch.optim.Adam on x, K = 4 models, `backward(retain_graph=True)`, the x_best / loss_best bookkeeping.
  Per-step x, posteriors, best loss and plan against the reference's own trace (g6), at test_g6_search_traces' bounds."""
  g = golden("g6_rip.npz")
  models = [hip_model(100 + k, dev) for k in range(4)]
  for os_ in (60, 61, 62):
    tag = "%s_o%d" % (algo, os_)
    ob = synth_observation(np.random.default_rng(os_))
    zs = [torch.from_numpy(g["zs_" + tag][k:k + 1].copy()).to(dev) for k in range(4)]
    goal = torch.from_numpy(ob["goal"][None, :, :2].copy()).to(dev)
    x = torch.zeros(1, 4, 2, device=dev, requires_grad=True)
    optimizer = torch.optim.Adam([x], lr=0.1)
    x_best = x.clone()
    loss_best = torch.ones((), device=dev) * 1000.0
    xs, posts = [], []
    for _ in range(10):
      optimizer.zero_grad()
      y, _ = models[0]._forward(x=x, z=zs[0])
      post = []
      for model, z in zip(models, zs):
        _, log_prob, logabsdet = model._inverse(y=y, z=z)
        post.append(torch.mean(log_prob - logabsdet) + model._goal_likelihood(y=y, goal=goal, epsilon=1.0))
      post = torch.stack(post, dim=0)
      loss = _aggregate(-post, algo)
      loss.backward(retain_graph=True)
      optimizer.step()
      if loss < loss_best:
        x_best = x.clone()
        loss_best = loss.clone()
      xs.append(x.detach().cpu().numpy()[0].copy())
      posts.append(post.detach().cpu().numpy())
    plan, _ = models[0]._forward(x=x_best, z=zs[0])
    err = float(np.abs(np.stack(xs) - g["x_" + tag]).max())
    print("rip autograd %s: max|dx| over the steps = %.3g" % (tag, err))
    np.testing.assert_allclose(np.stack(posts), g["post_" + tag], rtol=1e-5, atol=3e-4)
    np.testing.assert_allclose(np.stack(xs), g["x_" + tag], atol=TOL)
    np.testing.assert_allclose(float(loss_best), float(g["loss_best_" + tag]), rtol=1e-5, atol=3e-4)
    np.testing.assert_allclose(plan.detach().cpu().numpy()[0], g["plan_" + tag], atol=TOL)


def test_reference_dim_recipe_through_autograd(golden, dev):
  """ImitativeModel.forward's loop (dim/model.py:100-139) through autograd on this package's methods: B = 1 and 3, with
  and without a goal, lr 5e-2, 20 steps, the g7 start and z; the final plan against the reference's (g7)."""
  g = golden("g7_dim_forward.npz")
  m = hip_model(7, dev)
  for B, os_ in ((1, 70), (3, 71)):
    obs_list = [synth_observation(np.random.default_rng(os_ + 10 * b)) for b in range(B)]
    goal = torch.stack([torch.from_numpy(o["goal"][:, :2].copy()) for o in obs_list]).to(dev)
    z = torch.from_numpy(g["z_B%d" % B]).to(dev)
    for with_goal in (0, 1):
      tag = "B%d_goal%d" % (B, with_goal)
      x = torch.from_numpy(g["x0_" + tag]).to(dev).repeat(B, 1).view(B, 4, 2)
      x.requires_grad = True
      optimizer = torch.optim.Adam([x], lr=5e-2)
      x_best = x.clone()
      loss_best = torch.ones((), device=dev) * 1000.0
      for _ in range(20):
        optimizer.zero_grad()
        y, _ = m._decoder._forward(x=x, z=z)
        _, log_prob, logabsdet = m._decoder._inverse(y=y, z=z)
        imitation_prior = torch.mean(log_prob - logabsdet)
        goal_likelihood = m._goal_likelihood(y=y, goal=goal, epsilon=1.0) if with_goal else 0.0
        loss = -(imitation_prior + goal_likelihood)
        loss.backward(retain_graph=True)
        optimizer.step()
        if loss < loss_best:
          x_best = x.clone()
          loss_best = loss.clone()
      y, _ = m._decoder._forward(x=x_best, z=z)
      err = float(np.abs(y.detach().cpu().numpy() - g["y_" + tag]).max())
      print("dim autograd %s: max|dy| = %.3g" % (tag, err))
      np.testing.assert_allclose(y.detach().cpu().numpy(), g["y_" + tag], atol=TOL)


def test_graph_mode_invariants(golden, dev):
  """Graph-building calls return the no-grad bits; a retained graph gives the same gradient bits twice; the broadcast-z
  gradient is the same bits on every run and equals the sum of the per-row gradients."""
  g = golden("g2_flow.npz")
  m = hip_model(int(g["weight_seed"]), dev)
  x, y, z = (torch.from_numpy(g[k]).to(dev) for k in ("x", "y", "z"))
  goal = torch.from_numpy(golden("g4_goal.npz")["goal"]).to(dev)
  with torch.no_grad():
    want = list(m._forward(x, z)) + list(m._inverse(y, z)) + [m._goal_likelihood_rows(y, goal)]
  xg, yg, zg = x.clone().requires_grad_(), y.clone().requires_grad_(), z.clone().requires_grad_()
  got = list(m._forward(xg, zg)) + list(m._inverse(yg, zg)) + [m._goal_likelihood_rows(yg, goal)]
  for a, b in zip(got, want):
    assert a.grad_fn is not None and torch.equal(a.detach(), b)

  rng = np.random.default_rng(5)
  gy = torch.from_numpy(rng.standard_normal((128, 4, 2)).astype(np.float32)).to(dev)
  y_out, lad = m._forward(xg, zg)
  _, lp, lad_i = m._inverse(y_out, zg)
  loss = (y_out * gy).sum() + lad.sum() - (lp - lad_i).sum() + m._goal_likelihood(y_out, goal)
  loss.backward(retain_graph=True)
  g1 = (xg.grad.clone(), zg.grad.clone())
  xg.grad, zg.grad = None, None
  loss.backward()
  assert torch.equal(xg.grad, g1[0]) and torch.equal(zg.grad, g1[1])

  # broadcast z at N = 4096: deterministic, and the sum of the per-row gradients
  n = 4096
  xs = x.repeat(n // 128, 1, 1) + 0.1 * torch.randn(n, 4, 2, device=dev, generator=torch.Generator(dev).manual_seed(3))
  gx = torch.randn(n, 4, 2, device=dev, generator=torch.Generator(dev).manual_seed(4))
  z1 = z[:1].clone().requires_grad_()
  runs = []
  for _ in range(3):
    out, lad = m._forward(xs, z1)
    runs.append(torch.autograd.grad([out, lad], [z1], [gx, torch.ones(n, device=dev)])[0])
  assert all(torch.equal(r, runs[0]) for r in runs[1:])
  zr = z[:1].expand(n, 64).contiguous().requires_grad_()
  out, lad = m._forward(xs, zr)
  per_row = torch.autograd.grad([out, lad], [zr], [gx, torch.ones(n, device=dev)])[0]
  np.testing.assert_allclose(runs[0].cpu().numpy()[0], per_row.double().sum(0).cpu().numpy(),
                             rtol=1e-5, atol=1e-5 * float(per_row.abs().sum(0).max()))


  # gradients in the input's dtype and shape: float64 inputs, broadcast z
  x64, z64 = x.double().requires_grad_(), z[:1].double().requires_grad_()
  out, lad = m._forward(x64, z64)
  (out.sum() + lad.sum()).backward()
  assert x64.grad.dtype == torch.float64 and x64.grad.shape == (128, 4, 2)
  assert z64.grad.dtype == torch.float64 and z64.grad.shape == (1, 64)


# The side-stream check runs in a child process: launches on a second hardware queue move the XCD that later launches of
# the SAME process start their workgroups on, and the one-launch encoder's placement probe (test_gpu_parity.py), which
# runs later in this pytest process, needs workgroup i on XCD i % 8.
_SIDE_STREAM_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from oatomobile_amd import ImitativeModel
dev = torch.device("cuda", 0)
g = np.load("tests/golden/g2_flow.npz")
m = ImitativeModel.synthetic(int(g["weight_seed"])).to(dev)
n = 4096
xs = torch.from_numpy(g["x"]).to(dev).repeat(n // 128, 1, 1)
gx = torch.randn(n, 4, 2, device=dev, generator=torch.Generator(dev).manual_seed(4))
z1 = torch.from_numpy(g["z"][:1].copy()).to(dev).requires_grad_()
out, lad = m._forward(xs, z1)
want = torch.autograd.grad([out, lad], [z1], [gx, torch.ones(n, device=dev)])[0]
s = torch.cuda.Stream(dev)
s.wait_stream(torch.cuda.current_stream(dev))
with torch.cuda.stream(s):
  out, lad = m._forward(xs, z1)
  side = torch.autograd.grad([out, lad], [z1], [gx, torch.ones(n, device=dev)])[0]
s.synchronize()
assert torch.equal(side, want), float((side - want).abs().max())
print("side stream ok")
"""


def test_backward_on_a_side_stream():
  """The backward runs on the forward's stream: forward and backward issued on a side stream give the default stream's
  bits (in a child process, see _SIDE_STREAM_CHILD)."""
  r = subprocess.run([sys.executable, "-c", _SIDE_STREAM_CHILD], cwd=ROOT, capture_output=True, text=True, timeout=300)
  assert r.returncode == 0 and "side stream ok" in r.stdout, r.stdout + r.stderr


def test_refusals_and_cpu_tensors(golden, dev):
  """Gradients do not reach model parameters or goals: such graph-building calls raise instead of returning an
  incomplete graph.  CPU tensors still raise (no CPU path)."""
  g = golden("g2_flow.npz")
  m = hip_model(int(g["weight_seed"]), dev)
  x, y, z = (torch.from_numpy(g[k]).to(dev) for k in ("x", "y", "z"))
  p = next(m._decoder.parameters())
  p.requires_grad_(True)
  try:
    with pytest.raises(RuntimeError, match="do not reach model parameters"):
      m._forward(x.clone().requires_grad_(), z)
    with pytest.raises(RuntimeError, match="do not reach model parameters"):
      m._decoder._inverse(y, z.clone().requires_grad_())
    with torch.no_grad():  # not a graph-building call: unchanged
      m._forward(x.clone().requires_grad_(), z)
  finally:
    p.requires_grad_(False)
  goal = torch.from_numpy(golden("g4_goal.npz")["goal"]).to(dev)
  with pytest.raises(RuntimeError, match="do not reach goals"):
    m._goal_likelihood(y.clone().requires_grad_(), goal.clone().requires_grad_())
  with pytest.raises(RuntimeError, match="do not reach goals"):
    m._goal_likelihood_rows(y, goal.clone().requires_grad_())
  for call in (lambda: m._forward(x.cpu().requires_grad_(), z.cpu()),
               lambda: m._inverse(y.cpu().requires_grad_(), z.cpu()),
               lambda: m._goal_likelihood(y.cpu().requires_grad_(), goal.cpu())):
    with pytest.raises(RuntimeError, match="no CPU path"):
      call()


def test_abi_validation(golden, dev):
  """rip_flow_vjp / rip_goal_likelihood_vjp: RIP_EINVAL on NULL or bad shapes, nothing launched for N = 0, z_rows = 1
  with and without a workspace."""
  from oatomobile_amd import _lib
  lib = _lib.load()
  g = golden("g2_flow.npz")
  m = hip_model(int(g["weight_seed"]), dev)
  h = m._handle()
  P = _lib.ptr
  x, z = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["z"]).to(dev)
  gy = torch.ones(128, 4, 2, device=dev)
  dx, dz = torch.empty(128, 4, 2, device=dev), torch.empty(1, 64, device=dev)
  ws_bytes = lib.rip_flow_vjp_workspace_bytes(128, 1)
  assert ws_bytes == 32 * 4 * 64 * 4 and lib.rip_flow_vjp_workspace_bytes(128, 128) == 0
  assert lib.rip_flow_vjp_workspace_bytes(1, 1) == 0 and lib.rip_flow_vjp_workspace_bytes(0, 1) == 0
  ws = torch.empty(ws_bytes // 4, device=dev)

  def vjp(mode=0, inp=x, zz=z[:1], n=128, z_rows=1, ga=gy, glp=None, glad=None, d_in=dx, d_z=dz, w=ws):
    return lib.rip_flow_vjp(h.raw, 0, mode, P(inp), P(zz), n, z_rows, P(ga), P(glp), P(glad), P(d_in), P(d_z), P(w),
                            h.stream())

  assert vjp(inp=None) == _lib.RIP_EINVAL
  assert vjp(zz=None) == _lib.RIP_EINVAL
  assert vjp(mode=2) == _lib.RIP_EINVAL
  assert vjp(z_rows=2) == _lib.RIP_EINVAL
  assert vjp(n=-1) == _lib.RIP_EINVAL
  assert vjp(glp=torch.ones(128, device=dev)) == _lib.RIP_EINVAL  # no log_prob in forward mode
  assert vjp(w=None) == _lib.RIP_EINVAL  # broadcast dz needs the workspace
  assert lib.rip_flow_vjp(None, 0, 0, P(x), P(z), 128, 128, None, None, None, P(dx), None, None, None) == _lib.RIP_EINVAL
  assert lib.rip_flow_vjp(h.raw, 1, 0, P(x), P(z), 128, 128, None, None, None, P(dx), None, None, None) == _lib.RIP_EINVAL

  sentinel = torch.full((1, 64), 7.0, device=dev)
  assert vjp(n=0, d_in=None, d_z=sentinel, w=None) == 0
  torch.cuda.synchronize(dev)
  assert torch.equal(sentinel, torch.full((1, 64), 7.0, device=dev))

  # z_rows = 1: N = 1 needs no workspace, N = 128 does; both agree with autograd through the method
  zg = z[:1].clone().requires_grad_()
  for n in (1, 128):
    out, _ = m._forward(x[:n], zg)
    (want,) = torch.autograd.grad(out, [zg], [gy[:n]])
    d_z = torch.empty(1, 64, device=dev)
    assert vjp(inp=x[:n].contiguous(), n=n, ga=gy[:n].contiguous(), d_in=None, d_z=d_z, w=None if n == 1 else ws) == 0
    assert torch.equal(d_z, want)

  goal = torch.from_numpy(golden("g4_goal.npz")["goal"]).to(dev)
  grow, dy = torch.ones(128, device=dev), torch.empty(128, 4, 2, device=dev)
  gv = lib.rip_goal_likelihood_vjp
  s = _lib.current_stream(dev)
  assert gv(P(x), None, 128, 128, 10, 1.0, P(grow), P(dy), s) == _lib.RIP_EINVAL
  assert gv(P(x), P(goal), 128, 128, 10, 1.0, None, P(dy), s) == _lib.RIP_EINVAL
  assert gv(P(x), P(goal), 128, 128, 10, 1.0, P(grow), None, s) == _lib.RIP_EINVAL
  assert gv(P(x), P(goal), 128, 3, 10, 1.0, P(grow), P(dy), s) == _lib.RIP_EINVAL
  assert gv(P(x), P(goal), 128, 128, 0, 1.0, P(grow), P(dy), s) == _lib.RIP_EINVAL
  assert gv(P(x), P(goal), 128, 128, 10, 0.0, P(grow), P(dy), s) == _lib.RIP_EINVAL
  dy.fill_(7.0)
  assert gv(P(x), P(goal), 0, 1, 10, 1.0, P(grow), P(dy), s) == 0
  torch.cuda.synchronize(dev)
  assert bool((dy == 7.0).all())
