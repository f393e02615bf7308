"""What the ensemble-disagreement statistics cost (rip_plan_stats / rip_act_stats: ensemble_stats_kernel).

  python tools/plan_stats_time.py [--out profiles/plan_stats/plan_stats_time.json]
  python tools/plan_stats_time.py --kernel-only      # the launches alone, for a `rocprofv3 --kernel-trace --stats` run

Three measurements, nothing compared against a target:
  * the batch unit of the README headline with the inputs resident in HBM — K = 4, N = 128, 2048 observations per step,
    bf16 encoder, `plan_batch(interpolate=True)` — with and without `return_stats`, the two alternating in one process:
    median of three 20-step regions each, device events, after warm-up;
  * `agent(observation)` (one captured hipGraph per call) with `stats=True` against `stats=False`: p50 of the host wall
    time per call over `--calls` calls each, in alternating blocks of 250;
  * `rip_plan_stats` alone at B = 2048 and B = 1 (K = 4, M = 1), device events, median of `--iters` launches.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oatomobile_amd import ImitativeModel, RIPAgent, _lib  # noqa: E402
from tests.helpers import synth_observation  # noqa: E402


def device_batch(B, dev, seed=0, C=2, G=10):
  """B synthetic observations built on the device, distributed like tests.helpers.synth_observation."""
  gen = torch.Generator(dev).manual_seed(seed)
  levels = torch.randint(0, 6, (B, 200, 200, C), device=dev, generator=gen).float() / 5.0
  lidar = levels * (torch.rand((B, 200, 200, C), device=dev, generator=gen) < 0.12)
  vec = torch.cat([torch.randn((B, 3), device=dev, generator=gen) * 3.0,
                   (torch.rand((B, 1), device=dev, generator=gen) < 0.2).float(),
                   torch.randint(0, 4, (B, 1), device=dev, generator=gen).float()], dim=1)
  goal = torch.cumsum(torch.randn((B, G, 2), device=dev, generator=gen).abs() * 2.0, dim=1)
  return lidar.contiguous(), vec.contiguous(), goal.contiguous()


def region_ms(fn, steps):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(steps):
    fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) / steps


def stats_launches(agent, dev, iters, res=None):
  lib, P, h = _lib.load(), _lib.ptr, agent._handle
  K = len(agent._models)
  gen = torch.Generator(dev).manual_seed(1)
  for B in (2048, 1):
    z = torch.randn(K, B, 64, device=dev, generator=gen)
    y = torch.cumsum(torch.randn(B, 1, 4, 2, device=dev, generator=gen).abs() * 1.5, dim=2).contiguous()
    q, st = torch.empty(K, B, 1, device=dev), torch.empty(B, 1, 4, device=dev)
    ms = []
    for i in range(iters + 3):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      _lib.check(lib.rip_plan_stats(h.raw, P(z), P(y), B, 1, P(q), P(st), h.stream()))
      b.record()
      b.synchronize()
      if i >= 3:
        ms.append(a.elapsed_time(b))
    if res is not None:
      res["rip_plan_stats_K%d_B%d_us" % (K, B)] = dict(median=1e3 * float(np.median(ms)), min=1e3 * float(np.min(ms)))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=2048)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--calls", type=int, default=3000)
  ap.add_argument("--iters", type=int, default=50)
  ap.add_argument("--kernel-only", action="store_true")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_stats", "plan_stats_time.json"))
  args = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  dev = torch.device("cuda", 0)
  torch.cuda.set_device(dev)
  K, N, B = 4, 128, args.batch
  models = [ImitativeModel.synthetic(100 + k).to(dev) for k in range(K)]
  if args.kernel_only:
    agent = RIPAgent(None, algorithm="WCM", models=models, max_batch=1)
    stats_launches(agent, dev, 10)
    torch.cuda.synchronize()
    return
  res = dict(device=torch.cuda.get_device_name(dev), K=K, N=N, batch=B, steps_per_region=args.steps)

  # -- the batch unit, with and without the statistics, alternating -------------------------------------------------
  agent = RIPAgent(None, algorithm="WCM", models=models, num_candidates=N, max_batch=B, encoder_dtype="bf16")
  lidar, vec, goal = device_batch(B, dev)
  out = torch.empty(B, 30, 3, device=dev, dtype=torch.float64)
  plain = lambda: agent.plan_batch(lidar, vec, goal, interpolate=True, out=out)
  with_stats = lambda: agent.plan_batch(lidar, vec, goal, interpolate=True, out=out, return_stats=True)
  for _ in range(3):
    plain()
    with_stats()
  torch.cuda.synchronize()
  regions = dict(plain=[], stats=[])
  for _ in range(3):
    regions["plain"].append(region_ms(plain, args.steps))
    regions["stats"].append(region_ms(with_stats, args.steps))
  res["plan_batch_ms_per_step"] = {k: dict(median=float(np.median(v)), regions=v) for k, v in regions.items()}
  res["plan_batch_stats_cost_ms"] = res["plan_batch_ms_per_step"]["stats"]["median"] - res["plan_batch_ms_per_step"]["plain"]["median"]
  ps = agent.plan_batch(lidar, vec, goal, return_stats=True)[1]
  res["variance_over_the_batch"] = dict(min=float(ps.variance.min()), median=float(ps.variance.median()), max=float(ps.variance.max()))
  stats_launches(agent, dev, args.iters, res)
  del agent, lidar, out

  # -- the online path ----------------------------------------------------------------------------------------------
  agents = dict(plain=RIPAgent(None, algorithm="WCM", models=models, num_candidates=N),
                stats=RIPAgent(None, algorithm="WCM", models=models, num_candidates=N, stats=True))
  obs = [synth_observation(np.random.default_rng(60 + i)) for i in range(8)]
  for a in agents.values():
    for i in range(50):
      a(obs[i % 8])
  wall = dict(plain=[], stats=[])
  block = 250
  for c0 in range(0, args.calls, block):
    for name, a in agents.items():
      for i in range(block):
        t0 = time.perf_counter()
        a(obs[i % 8])
        wall[name].append(time.perf_counter() - t0)
  res["online_us"] = {k: dict(p50=1e6 * float(np.percentile(v, 50)), p90=1e6 * float(np.percentile(v, 90)), calls=len(v))
                      for k, v in wall.items()}
  res["online_graph_captured"] = {k: next(iter(a._online.values()))["graph"] is not None for k, a in agents.items()}
  res["online_stats_cost_us_p50"] = res["online_us"]["stats"]["p50"] - res["online_us"]["plain"]["p50"]
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
  print(json.dumps(res))


if __name__ == "__main__":
  main()
