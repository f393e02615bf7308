"""What adapting a K = 4 ensemble costs, the new road beside the existing one, at B = 128 and 512 in one process:

  head_step      `HeadTrainer.train_step` on cached features: forward / backward + Adam of the K heads (four launches)
  dim_steps      K x `DIMTrainer.train_step` on the same rows (the whole network per member, train-mode BatchNorm)
  cache_build    `FeatureCache.build` per 1 000 observations (batches of 128 through the K encoders)
  publish        `HeadTrainer.publish` per member (the device repack of a whole member, `rip_load_model_device`)

Device events around `steps` calls after `warmup` ones, the configurations taking turns region by region; the median of
`rounds` regions and their spread (min .. max).  Nothing is gated.  One JSON line on stdout, a copy under --out.

    python tools/head_train_time.py [--steps 10] [--warmup 3] [--rounds 7] [--out profiles/head_train/head_train_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 4


def region(fn, steps):
  import torch
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(steps):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / steps


def summary(ts, digits=4):
  return {"median_ms": round(float(np.median(ts)), digits), "min_max_ms": [round(min(ts), digits), round(max(ts), digits)]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_train", "head_train_time.json"))
  a = ap.parse_args()
  import torch
  from oatomobile_amd import DIMTrainer, ImitativeModel, RIPAgent, replay
  from oatomobile_amd.train import HeadTrainer
  if not torch.cuda.is_available():
    raise SystemExit("head_train_time.py needs a GPU")
  dev = torch.device("cuda", 0)
  rng = np.random.default_rng(77)
  n, L = 1000, 8
  codes = (rng.integers(0, 6, size=(n, 200, 200, 2)) * (rng.random((n, 200, 200, 2)) < 0.12)).astype(np.uint8)
  lut = np.zeros(256, np.float32)
  lut[:6] = np.arange(6, dtype=np.float32) / 5.0
  vec = np.concatenate([rng.normal(0, 3.0, (n, 3)), rng.random((n, 1)) < 0.2, rng.integers(0, 4, (n, 1))], axis=1).astype(np.float32)
  future = np.cumsum(np.abs(rng.normal(size=(n, L, 2))) * 0.5, axis=1).astype(np.float32)
  data = replay.DeviceCache.from_tensors(torch.from_numpy(codes).to(dev), torch.from_numpy(lut).to(dev), torch.from_numpy(vec).to(dev),
                                         torch.from_numpy(future).to(dev), torch.zeros(n, device=dev))
  models = [ImitativeModel.synthetic(100 + k) for k in range(K)]
  agent = RIPAgent(None, algorithm="WCM", models=models, num_candidates=16, max_batch=128, device=dev)
  out = {"K": K, "steps_per_region": a.steps, "regions": a.rounds, "device": torch.cuda.get_device_name(0)}

  builds = []
  cache = replay.FeatureCache.build(agent, data, 128)  # warm-up
  torch.cuda.synchronize()
  for _ in range(a.rounds):
    builds.append(region(lambda: replay.FeatureCache.build(agent, data, 128), 1))
  out["cache_build_per_1000_observations"] = summary(builds, 3)

  head = HeadTrainer(agent, lr=1e-3, max_batch=512)
  dims = [DIMTrainer(ImitativeModel.synthetic(100 + k, max_batch=1).to(dev), lr=1e-3, max_batch=512, device=dev) for k in range(K)]
  for B in (128, 512):
    rows = torch.from_numpy(rng.integers(0, n, size=(K, B))).to(dev)
    shared = rows[0].contiguous()
    batch = data.batch(shared, 4)

    def head_step():
      head.train_step(cache.feat, cache.vec, target=cache.future, rows=rows)

    def dim_steps():
      for tr in dims:
        tr.train_step(batch)

    for fn in (head_step, dim_steps):
      for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    times = {"head_step": [], "dim_steps": []}
    for _ in range(a.rounds):
      times["head_step"].append(region(head_step, a.steps))
      times["dim_steps"].append(region(dim_steps, a.steps))
    out["b%d" % B] = {"head_step_K_members": summary(times["head_step"]), "K_dim_train_steps": summary(times["dim_steps"])}

  head.publish(agent)  # warm-up
  torch.cuda.synchronize()
  pubs = [region(lambda: head.publish(agent), 1) / K for _ in range(a.rounds)]
  out["publish_per_member"] = summary(pubs)
  line = json.dumps(out)
  print(line)
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  with open(a.out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()
