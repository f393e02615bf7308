"""Times of the two roads from a `DIMTrainer` to a live `RIPAgent` (reported, not gated), K = 4 members, both roads in
one process, alternating.  One JSON line on stdout, and the same line into `--out` (default
profiles/publish/publish_time.json); every figure is the median of `--rounds` rounds with its min .. max:

  host_road_ms_per_member     (a) `trainer.sync_to_model()` for every member + `agent.refresh()`, synchronised, / K:
                              328 tensors to the host, the numpy flattening, the BatchNorm fold and the seven re-layouts
                              on one CPU thread, a device-wide synchronise and eight blocking copies per member
  first_call_after_host_ms    the first `agent(observation)` behind it (re-captures the one-observation pipeline)
  device_road_ms_per_member   (b) `agent.load_member(k, trainer)` for every member, synchronised, / K
  first_call_after_device_ms  the first `agent(observation)` behind it (replays the pipeline captured before)
  load_device_us_per_member   (c) `Handle.load_model_device` alone: four launches and the flag read, wall clock per call
  load_device_kernels_us      ... the same calls between two device events (the kernels without the host's share)
  online_call_ms              `agent(observation)` with nothing loaded in between, for scale

    python tools/publish_time.py [--rounds 9] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, TRAIN_B = 4, 3


def spread(ts, scale=1.0, digits=3):
  return {"median": round(float(np.median(ts)) * scale, digits), "min_max": [round(min(ts) * scale, digits), round(max(ts) * scale, digits)]}


def train_batch(dev, seed):
  import torch
  from oatomobile_amd import arch, transform_visual
  rng = np.random.default_rng(seed)
  lidar = ((rng.integers(0, 6, size=(TRAIN_B, 200, 200, 2)) / 5.0) * (rng.random((TRAIN_B, 200, 200, 2)) < 0.12)).astype(np.float32)
  future = np.cumsum(np.abs(rng.normal(size=(TRAIN_B, arch.T, 2))) * 0.5, axis=1).astype(np.float32)
  return dict(visual_features=transform_visual(torch.from_numpy(lidar).to(dev), channels_last=True),
              velocity=torch.from_numpy(rng.normal(0, 3.0, size=(TRAIN_B, 3)).astype(np.float32)).to(dev),
              is_at_traffic_light=torch.zeros(TRAIN_B, 1, device=dev), traffic_light_state=torch.ones(TRAIN_B, 1, device=dev),
              player_future=torch.from_numpy(future).to(dev))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=9)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "publish", "publish_time.json"))
  a = ap.parse_args()
  import torch
  from oatomobile_amd import DIMTrainer, ImitativeModel, RIPAgent
  from tests.helpers import synth_observation
  if not torch.cuda.is_available():
    raise SystemExit("publish_time.py needs a GPU")
  dev = torch.device("cuda", 0)
  torch.cuda.set_device(dev)
  models = [ImitativeModel.synthetic(700 + k).to(dev) for k in range(K)]
  agent = RIPAgent(None, algorithm="WCM", models=models, num_candidates=16, seed=0)
  trainers = [DIMTrainer(m, lr=1e-3, max_batch=4, device=dev) for m in models]
  ob = synth_observation(np.random.default_rng(1))
  sync = lambda: torch.cuda.synchronize(dev)
  host, host_call, device, device_call, load, kernels, online = [], [], [], [], [], [], []
  for r in range(a.rounds + 1):  # the first round warms up
    for k, tr in enumerate(trainers):
      tr.train_step(train_batch(dev, 100 * r + k))  # the weights really change between rounds
    sync()
    t0 = time.perf_counter()
    for tr in trainers:
      tr.sync_to_model()
    agent.refresh()
    sync()
    t1 = time.perf_counter()
    plan_host = agent(dict(ob))
    t2 = time.perf_counter()
    host.append((t1 - t0) / K)
    host_call.append(t2 - t1)
    t0 = time.perf_counter()
    for k, tr in enumerate(trainers):
      agent.load_member(k, tr)
    sync()
    t1 = time.perf_counter()
    plan_device = agent(dict(ob))
    t2 = time.perf_counter()
    device.append((t1 - t0) / K)
    device_call.append(t2 - t1)
    assert np.array_equal(plan_host, plan_device), "the two roads gave different plans"
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for k, tr in enumerate(trainers):
      agent._handle.load_model_device(k, tr.params)
    e1.record()
    sync()
    load.append((time.perf_counter() - t0) / K)
    kernels.append(e0.elapsed_time(e1) / K)
    ts = []
    for _ in range(20):
      t0 = time.perf_counter()
      agent(dict(ob))
      ts.append(time.perf_counter() - t0)
    online.append(float(np.median(ts)))
  out = {"device": torch.cuda.get_device_name(0), "members": K, "rounds": a.rounds,
         "host_road_ms_per_member": spread(host[1:], 1e3), "first_call_after_host_ms": spread(host_call[1:], 1e3),
         "device_road_ms_per_member": spread(device[1:], 1e3), "first_call_after_device_ms": spread(device_call[1:], 1e3),
         "load_device_us_per_member": spread(load[1:], 1e6, 1), "load_device_kernels_us": spread(kernels[1:], 1e3, 1),
         "online_call_ms": spread(online[1:], 1e3)}
  line = json.dumps(out)
  print(line)
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  with open(a.out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()
