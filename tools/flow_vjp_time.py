"""Device-event timing of the flow VJP kernels (rip_flow_vjp) beside the plain inverse, and of one autograd step of the
reference RIP recipe (rip/agent.py:85-137 written against this package's methods) beside one fused rip_search step.

  python tools/flow_vjp_time.py [--rows 65536] [--iters 20] [--out profiles/flow_autograd/flow_vjp_time.json]

Rows default to 65 536 = 512 observations x 128 candidates.  Every timing is the median over `--iters` event-timed
launches after warm-up; nothing here is compared against a target.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oatomobile_amd import ImitativeModel, RIPAgent, _lib  # noqa: E402
from tests.helpers import synth_observation  # noqa: E402


def timed(fn, iters, warmup=3):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  ms = []
  for _ in range(iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b))
  return float(np.median(ms)), float(np.min(ms))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rows", type=int, default=512 * 128)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_autograd", "flow_vjp_time.json"))
  args = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  dev = torch.device("cuda", 0)
  torch.cuda.set_device(dev)
  lib = _lib.load()
  P = _lib.ptr
  n = args.rows
  gen = torch.Generator(dev).manual_seed(0)
  m = ImitativeModel.synthetic(100).to(dev)
  h = m._handle()
  x = torch.randn(n, 4, 2, device=dev, generator=gen)
  res = dict(device=torch.cuda.get_device_name(dev), rows=n, iters=args.iters, unit="ms (median, min)")
  for z_rows in (n, 1):
    z = torch.randn(z_rows, 64, device=dev, generator=gen)
    with torch.no_grad():
      y, _ = m._forward(x, z)
    xo, lp, lad = torch.empty_like(y), torch.empty(n, device=dev), torch.empty(n, device=dev)
    gy, g1, g2 = torch.randn(n, 4, 2, device=dev, generator=gen), torch.randn(n, device=dev, generator=gen), torch.randn(
        n, device=dev, generator=gen)
    d_in, dz = torch.empty(n, 4, 2, device=dev), torch.empty(z_rows, 64, device=dev)
    ws_bytes = lib.rip_flow_vjp_workspace_bytes(n, z_rows)
    ws = torch.empty(max(ws_bytes // 4, 1), device=dev)
    tag = "z_rows_N" if z_rows == n else "z_rows_1"
    res["inverse_" + tag] = timed(lambda: _lib.check(lib.rip_flow_inverse(
        h.raw, 0, P(y), P(z), n, z_rows, P(xo), P(lp), P(lad), h.stream())), args.iters)
    res["vjp_forward_" + tag] = timed(lambda: _lib.check(lib.rip_flow_vjp(
        h.raw, 0, 0, P(x), P(z), n, z_rows, P(gy), None, P(g2), P(d_in), P(dz), P(ws), h.stream())), args.iters)
    res["vjp_inverse_" + tag] = timed(lambda: _lib.check(lib.rip_flow_vjp(
        h.raw, 0, 1, P(y), P(z), n, z_rows, P(gy), P(g1), P(g2), P(d_in), P(dz), P(ws), h.stream())), args.iters)
    res["vjp_inverse_dy_only_" + tag] = timed(lambda: _lib.check(lib.rip_flow_vjp(
        h.raw, 0, 1, P(y), P(z), n, z_rows, P(gy), P(g1), P(g2), P(d_in), None, None, h.stream())), args.iters)

  # one step of the reference RIP recipe through autograd (K = 4, B = 1) beside the fused search
  models = [ImitativeModel.synthetic(100 + k).to(dev) for k in range(4)]
  ob = synth_observation(np.random.default_rng(60))
  agent = RIPAgent(None, algorithm="WCM", models=models)
  agent(dict(ob))  # uploads the ensemble to the agent's handle
  zs = [torch.randn(1, 64, device=dev, generator=gen) for _ in range(4)]
  goal = torch.from_numpy(ob["goal"][None, :, :2].copy()).to(dev)
  x = torch.zeros(1, 4, 2, device=dev, requires_grad=True)
  opt = torch.optim.Adam([x], lr=0.1)

  def autograd_step():
    opt.zero_grad()
    y, _ = models[0]._forward(x=x, z=zs[0])
    post = []
    for model, z in zip(models, zs):
      _, log_prob, logabsdet = model._inverse(y=y, z=z)
      post.append(torch.mean(log_prob - logabsdet) + model._goal_likelihood(y=y, goal=goal, epsilon=1.0))
    loss, _ = torch.min(-torch.stack(post, dim=0), dim=0)
    loss.backward(retain_graph=True)
    opt.step()

  res["rip_autograd_step_K4_B1"] = timed(autograd_step, args.iters * 5)
  zk = torch.cat(zs, 0).reshape(4, 1, 64).contiguous()
  x0 = torch.zeros(1, 1, 4, 2, device=dev)
  plan = torch.empty(1, 4, 2, device=dev)
  G = goal.shape[1]
  for steps in (1, 10):
    res["rip_search_%dstep_K4_B1" % steps] = timed(lambda: _lib.check(lib.rip_search(
        agent._handle.raw, P(zk), P(goal), P(x0), 1, 1, G, 0, steps, 0.1, 1.0, P(plan), None, None, None, None, None,
        None, agent._handle.stream())), args.iters * 5)
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
  print(json.dumps(res))


if __name__ == "__main__":
  main()
