"""Observations/s of DIM training at batch 512 along three paths, on the same synthetic datum files:

  (a) step      `DIMTrainer.train_step` on one pre-assembled device batch (the ceiling: no data path at all);
  (b) epoch     `DIMTrainer.train_epoch` from a `replay.DeviceCache` (permutation, batch assembly on the GPU,
                target noise, dropout mask, step; one synchronisation per epoch);
  (c) loader    the reference's path (dim/train.py:122-160, 215-227): `replay.as_torch` + `DataLoader(shuffle=True,
                num_workers=min(14, effective_cpus() - 2))` + `.to(device)` + `ImitativeModel.transform` +
                `train_step`.

Also the batch assembly kernel's own time per batch (`DeviceCache.batch`, device events) against the gather-then-
transform copy it replaces (`codes[rows]` -> `lut[...]` -> `transform_visual`), with the bytes each moves.  Every
phase is bounded in steps.  One JSON line on stdout (and in --out).

    python tools/train_epoch_time.py [--n 2048] [--batch 512] [--epochs 3] [--steps 10] [--loader-steps 6]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _write(args):
  """Datum files i0..i1 (a worker process: numpy only, no GPU)."""
  d, i0, i1 = args
  from oatomobile_amd import replay
  from tests.helpers import synth_observation
  ep = replay.Episode(os.path.dirname(d), os.path.basename(d))
  for i in range(i0, i1):
    rng = np.random.default_rng(i)
    o = synth_observation(rng)
    fut = np.cumsum(np.abs(rng.normal(size=(80, 3))) * 0.3, axis=0).astype(np.float32)
    ep.append("d%06d" % i, lidar=o["lidar"], velocity=o["velocity"], is_at_traffic_light=o["is_at_traffic_light"],
              traffic_light_state=o["traffic_light_state"], player_future=fut)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--n", type=int, default=2048, help="datum files (one epoch)")
  ap.add_argument("--batch", type=int, default=512)
  ap.add_argument("--epochs", type=int, default=3, help="timed epochs of (b), after one warm-up epoch")
  ap.add_argument("--steps", type=int, default=10, help="timed steps of (a), after two warm-up steps")
  ap.add_argument("--loader-steps", type=int, default=6, help="timed steps of (c), after one warm-up step")
  ap.add_argument("--gather-reps", type=int, default=50)
  ap.add_argument("--workdir", default=None)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  from oatomobile_amd import replay
  work = a.workdir or tempfile.mkdtemp(prefix="train_epoch_time_")
  split = os.path.join(work, "train")
  files = sorted(f for f in (os.listdir(split) if os.path.isdir(split) else []) if f.endswith(".npz"))
  t0 = time.perf_counter()
  if len(files) < a.n:  # before torch touches the GPU: plain worker processes
    procs = max(1, min(16, replay.effective_cpus()))
    cuts = [a.n * k // procs for k in range(procs + 1)]
    with ProcessPoolExecutor(procs) as ex:
      list(ex.map(_write, [(split, c0, c1) for c0, c1 in zip(cuts[:-1], cuts[1:]) if c1 > c0]))
  files = sorted(os.path.join(split, f) for f in os.listdir(split) if f.endswith(".npz"))[:a.n]
  t_write = time.perf_counter() - t0
  import torch
  from oatomobile_amd import DIMTrainer, ImitativeModel, transform_visual
  if not torch.cuda.is_available():
    raise SystemExit("train_epoch_time.py needs a GPU")
  dev = torch.device("cuda", 0)
  B = a.batch
  t0 = time.perf_counter()
  cache = replay.pack_cache(files, os.path.join(work, "cache"), targets=True)
  t_pack = time.perf_counter() - t0
  t0 = time.perf_counter()
  data = replay.DeviceCache(cache, dev)
  t_upload = time.perf_counter() - t0
  out = {"batch": B, "n": len(data), "write_datums_s": t_write, "pack_s": t_pack, "upload_s": t_upload}

  def trainer():
    return DIMTrainer(ImitativeModel.synthetic(7, max_batch=1).to(dev), lr=1e-3, max_batch=B, device=dev)

  # (a) the bare step on one pre-assembled batch
  tr = trainer()
  rows = torch.arange(B, device=dev) % len(data)
  batch = data.batch(rows, 4)
  for _ in range(2):
    tr.train_step(batch)
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(a.steps):
    tr.train_step(batch)
  e1.record()
  torch.cuda.synchronize()
  ms = e0.elapsed_time(e1) / a.steps
  out["a_step_ms"] = ms
  out["a_step_obs_per_s"] = B / ms * 1e3
  del tr

  # (b) whole epochs from the device-resident cache (wall clock: the host loop is part of the path)
  tr = trainer()
  g = torch.Generator(device=dev).manual_seed(0)
  tr.train_epoch(data, B, generator=g)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  losses = [tr.train_epoch(data, B, generator=g) for _ in range(a.epochs)]
  dt = time.perf_counter() - t0
  steps = a.epochs * ((len(data) + B - 1) // B)
  out["b_epoch_steps"] = steps
  out["b_epoch_ms_per_step"] = dt / steps * 1e3
  out["b_epoch_obs_per_s"] = a.epochs * len(data) / dt
  out["b_epoch_losses"] = losses
  out["b_over_a"] = out["b_epoch_obs_per_s"] / out["a_step_obs_per_s"]
  del tr

  # the assembly kernel alone, and the gather-then-transform copy it replaces
  perm = torch.randperm(len(data), device=dev)[:B]
  lut = data.lut
  for _ in range(3):
    data.batch(perm, 4)
    transform_visual(lut[data.codes[perm].long()], channels_last=True)
  torch.cuda.synchronize()
  e0.record()
  for _ in range(a.gather_reps):
    data.batch(perm, 4)
  e1.record()
  torch.cuda.synchronize()
  out["gather_kernel_us_per_batch"] = e0.elapsed_time(e1) / a.gather_reps * 1e3
  e0.record()
  for _ in range(a.gather_reps):
    transform_visual(lut[data.codes[perm].long()], channels_last=True)
  e1.record()
  torch.cuda.synchronize()
  out["gather_then_transform_us_per_batch"] = e0.elapsed_time(e1) / a.gather_reps * 1e3
  hwc = data.H * data.W * data.C
  vis = data.C * 100 * 100 * 4
  # one launch: codes read once (plus the patch halo), visual written once; the copy: index_select (read + write the
  # codes), int64 indices (the .long() copy: read 1 B, write 8 B), the table lookup (read 8 B, write 4 B per cell),
  # the transform (read 4 B per cell, write the visual)
  out["gather_kernel_bytes_per_obs"] = hwc + vis
  out["gather_then_transform_bytes_per_obs"] = 2 * hwc + 9 * hwc + 12 * hwc + 4 * hwc + vis

  # (c) the reference's loader path, bounded
  tr = trainer()
  model = tr._model
  workers = max(0, min(14, replay.effective_cpus() - 2))
  ds = replay.as_torch(split, modalities=("lidar", "is_at_traffic_light", "traffic_light_state", "player_future",
                                          "velocity"))
  loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=True, num_workers=workers, drop_last=False)
  it = iter(loader)
  done, t0 = 0, None
  while done < a.loader_steps + 1:
    try:
      b = next(it)
    except StopIteration:
      it = iter(loader)
      continue
    b = model.transform({k: v.to(dev) for k, v in b.items()})
    tr.train_step(b)
    if t0 is None:  # after the warm-up step (and the workers' start)
      torch.cuda.synchronize()
      t0, obs = time.perf_counter(), 0
    else:
      obs += b["visual_features"].shape[0]
    done += 1
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  out["c_loader_workers"] = workers
  out["c_loader_steps"] = a.loader_steps
  out["c_loader_obs_per_s"] = obs / dt
  out["b_over_c"] = out["b_epoch_obs_per_s"] / out["c_loader_obs_per_s"]
  line = json.dumps(out)
  print(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
