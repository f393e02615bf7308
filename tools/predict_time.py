"""What sample-and-rank prediction costs (rip_predict: sample_forward_kernel, ensemble_stats_kernel, rank_kernel).

  python tools/predict_time.py [--out profiles/predict/predict_time.json]
  python tools/predict_time.py --kernel-only     # the launches alone, for a `rocprofv3 --kernel-trace --stats` run: the
                                                 # three kernels of rip_predict apart, next to the yardstick's two

At K = 4 members, S = 32 samples each (M = 128 candidates), B = 2048 observations, z resident in HBM; device events
around regions of `--region` back-to-back calls, median of `--iters` regions after warm-up:
  * `rip_predict` as a whole (generator on, no goal, with a target, top_k = 6);
  * its scoring launch alone, which is `rip_plan_stats` on the candidates it produced;
  * the yardstick — what the library could already do with the same trajectories: `rip_score` + `rip_aggregate_scores`
    on [B,128].
Nothing is compared against a target.
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


def region_us(fn, calls):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(calls):
    fn()
  b.record()
  b.synchronize()
  return 1e3 * a.elapsed_time(b) / calls


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=2048)
  ap.add_argument("--members", type=int, default=4)
  ap.add_argument("--samples", type=int, default=32)
  ap.add_argument("--top-k", type=int, default=6)
  ap.add_argument("--region", type=int, default=10)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--kernel-only", action="store_true")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict", "predict_time.json"))
  args = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  dev = torch.device("cuda", 0)
  torch.cuda.set_device(dev)
  K, S, B, top_k = args.members, args.samples, args.batch, args.top_k
  M = K * S
  models = [ImitativeModel.synthetic(100 + k).to(dev) for k in range(K)]
  agent = RIPAgent(None, algorithm="WCM", models=models, max_batch=1)
  lib, P, h = _lib.load(), _lib.ptr, agent._handle
  gen = torch.Generator(dev).manual_seed(1)
  z = torch.randn(K, B, 64, device=dev, generator=gen)
  target = torch.cumsum(torch.randn(B, 4, 2, device=dev, generator=gen).abs() * 1.5, dim=1).contiguous()
  y_all, q, stats = torch.empty(B, M, 4, 2, device=dev), torch.empty(K, B, M, device=dev), torch.empty(B, M, 4, device=dev)
  y_top, loss_top = torch.empty(B, top_k, 4, 2, device=dev), torch.empty(B, top_k, device=dev)
  index = torch.empty(B, top_k, device=dev, dtype=torch.int32)
  ade, fde = torch.empty(B, top_k, device=dev), torch.empty(B, top_k, device=dev)
  scores, loss = torch.empty(K, B, M, device=dev), torch.empty(B, M, device=dev)
  best = torch.empty(B, device=dev, dtype=torch.int32)
  algo = _lib.ALGORITHMS["WCM"]

  def predict():
    _lib.check(lib.rip_predict(h.raw, P(z), None, 0, 1.0, P(target), None, 7, 0, B, S, top_k, algo, P(y_all), P(q), P(stats), None,
                               P(y_top), P(loss_top), P(index, torch.int32), P(ade), P(fde), h.stream()))

  def score_launch():
    _lib.check(lib.rip_plan_stats(h.raw, P(z), P(y_all), B, M, P(q), P(stats), h.stream()))

  def yardstick():
    _lib.check(lib.rip_score(h.raw, 0, K, P(z), P(y_all), None, B, M, 0, 1.0, P(scores), h.stream()))
    _lib.check(lib.rip_aggregate_scores(P(scores), K, B, M, algo, P(loss), P(best, torch.int32), h.stream()))

  fns = dict(rip_predict=predict, scoring_launch=score_launch, rip_score_plus_aggregate=yardstick)
  for fn in fns.values():
    for _ in range(3):
      fn()
  torch.cuda.synchronize()
  if args.kernel_only:
    return
  res = dict(device=torch.cuda.get_device_name(dev), K=K, S=S, M=M, batch=B, top_k=top_k, calls_per_region=args.region)
  times = {name: [] for name in fns}
  for _ in range(args.iters):  # the three alternate, so that clock drift falls on all of them
    for name, fn in fns.items():
      times[name].append(region_us(fn, args.region))
  res["us_per_call"] = {name: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for name, v in times.items()}
  med = {name: res["us_per_call"][name]["median"] for name in fns}
  res["sampling_plus_ranking_us"] = med["rip_predict"] - med["scoring_launch"]
  res["rip_predict_over_yardstick"] = med["rip_predict"] / med["rip_score_plus_aggregate"]
  assert torch.equal(q, scores), "rip_predict's q is not rip_score's"
  res["min_ade_1"] = float(ade[:, 0].mean())
  res["min_ade_k"] = float(ade.min(1).values.mean())
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
  print(json.dumps(res))


if __name__ == "__main__":
  main()
