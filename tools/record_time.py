"""Times of hindsight labelling and on-device recording (reported, not gated).  One JSON line on stdout, and the same
line into `--out` (default profiles/record/record_time.json):

  append_us_per_tick         `DeviceRecorder.append` of a 200 x 200 x 2 observation already on the device, host wall
                             clock per call over `--ticks` calls with one synchronisation at the end (what a driving
                             loop pays: the copies of vec and pose plus one `rip_code_bev_u8` launch), median of
                             `--rounds` regions and their min .. max
  code_bev_us                the `rip_code_bev_u8` launch alone (device events around `--ticks` launches)
  cache_ms_1000_frames       `DeviceRecorder.cache()` of a 1 000-frame recording (L = 80, P = 20: 900 labelled rows):
                             one `rip_hindsight_targets` launch, the row compaction and the one synchronisation
  hindsight_us_900_windows   the `rip_hindsight_targets` launch alone (device events)
  pack_episodes_s / process_then_pack_cache_s   raw episodes -> packed cache with targets, both ways, on the same 200
                             raw frames (one episode, L = 80, P = 20, every frame a window: 100 rows), numpy path and one
                             packing process each; pack_episodes_device_s is the same with device labelling

    python tools/record_time.py [--ticks 200] [--rounds 7] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def track(n, seed):
  rng = np.random.default_rng(seed)
  yaw = 170.0 + np.cumsum(rng.normal(0.8, 1.5, size=n))
  rad = np.deg2rad(yaw)
  xy = np.array([250.0, -120.0]) + np.cumsum(np.c_[np.cos(rad), np.sin(rad)] * np.abs(rng.normal(0.8, 0.4, size=(n, 1))), axis=0)
  location = np.c_[xy, np.full(n, 1.5)].astype(np.float32)
  rotation = np.c_[rng.normal(0, 2, n), (yaw + 180.0) % 360.0 - 180.0, rng.normal(0, 1, n)].astype(np.float32)
  return location, rotation


def lidar_frames(n, seed):
  rng = np.random.default_rng(seed)
  return ((rng.integers(0, 6, size=(n, 200, 200, 2)) / 5.0) * (rng.random((n, 200, 200, 2)) < 0.12)).astype(np.float32)


def spread(ts, scale=1.0, digits=2):
  return {"median": round(float(np.median(ts)) * scale, digits), "min_max": [round(min(ts) * scale, digits), round(max(ts) * scale, digits)]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--ticks", type=int, default=200)
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "record", "record_time.json"))
  a = ap.parse_args()
  import torch
  from oatomobile_amd import _lib, replay
  if not torch.cuda.is_available():
    raise SystemExit("record_time.py needs a GPU")
  dev = torch.device("cuda", 0)
  lut = np.full((256,), np.nan, np.float32)
  lut[:6] = np.array([0.0, 0.2, 0.4, 0.6, 0.8, 1.0], np.float32)
  out = {"device": torch.cuda.get_device_name(0), "ticks_per_region": a.ticks, "regions": a.rounds}

  # --- append per tick, and the coding launch alone
  frames = torch.from_numpy(lidar_frames(8, 1)).to(dev)
  location, rotation = track(1000, 2)
  vel, light, state = np.zeros(3, np.float32), np.float32(0), np.float32(1)
  wall, launch = [], []
  for r in range(a.rounds + 1):  # the first region warms up
    rec = replay.DeviceRecorder(a.ticks, (200, 200, 2), lut, dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(a.ticks):
      rec.append(lidar=frames[i % 8], velocity=vel, is_at_traffic_light=light, traffic_light_state=state,
                 location=location[i % 1000], rotation=rotation[i % 1000])
    torch.cuda.synchronize(dev)
    wall.append((time.perf_counter() - t0) / a.ticks)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lib, st = _lib.load(), _lib.current_stream(dev)
    e0.record()
    for i in range(a.ticks):
      lib.rip_code_bev_u8(_lib.ptr(frames[i % 8]), 1, 200, 200, 2, _lib.ptr(rec.lut), 6, _lib.ptr(rec.codes[i], torch.uint8),
                          _lib.ptr(rec._miss, torch.int32), st)
    e1.record()
    torch.cuda.synchronize(dev)
    launch.append(e0.elapsed_time(e1) / a.ticks)
  out["append_us_per_tick"] = spread(wall[1:], 1e6)
  out["code_bev_us"] = spread(launch[1:], 1e3)

  # --- cache() of a 1 000-frame recording
  rec = replay.DeviceRecorder(1000, (200, 200, 2), lut, dev)
  for i in range(1000):
    rec.append(lidar=frames[i % 8], velocity=vel, is_at_traffic_light=light, traffic_light_state=state, location=location[i],
               rotation=rotation[i])
  wall, launch = [], []
  for r in range(a.rounds + 1):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    data = rec.cache()
    wall.append(time.perf_counter() - t0)
    rows = torch.from_numpy(rec.frames).to(dev)
    episode = torch.zeros(1000, dtype=torch.int32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    replay._hindsight_launch(rec.location, rec.rotation, episode, rows, 80, 20, 10, 8, {"future_xy", "mode"})
    e1.record()
    torch.cuda.synchronize(dev)
    launch.append(e0.elapsed_time(e1))
  assert len(data) == 900
  out["cache_ms_1000_frames"] = spread(wall[1:], 1e3, 3)
  out["hindsight_us_900_windows"] = spread(launch[1:], 1e3)  # includes the allocation of the two outputs

  # --- raw episodes -> packed cache, both ways, on the same 200 raw frames
  with tempfile.TemporaryDirectory() as tmp:
    raw = os.path.join(tmp, "raw")
    ep = replay.Episode(raw, "ep0")
    bev = lidar_frames(200, 3)
    for i in range(200):
      ep.append("s%04d" % i, lidar=bev[i], velocity=vel, is_at_traffic_light=np.int64(0), traffic_light_state=np.int64(1),
                location=location[i], rotation=rotation[i])
    t0 = time.perf_counter()
    direct = replay.pack_episodes(raw, os.path.join(tmp, "direct"), num_frame_skips=1)
    t1 = time.perf_counter()
    files = replay.process(raw, os.path.join(tmp, "datums"), num_frame_skips=1)
    t2 = time.perf_counter()
    via = replay.pack_cache(files, os.path.join(tmp, "via"), workers=1, targets=True)
    t3 = time.perf_counter()
    replay.pack_episodes(raw, os.path.join(tmp, "device"), num_frame_skips=1, device=dev)
    t4 = time.perf_counter()
    assert len(direct) == len(via) == 100
    for name in ("codes.npy", "future.npy", "mode.npy"):
      assert np.load(os.path.join(tmp, "direct", name)).tobytes() == np.load(os.path.join(tmp, "via", name)).tobytes()
    out["pack_episodes_s"] = round(t1 - t0, 3)
    out["process_then_pack_cache_s"] = {"process": round(t2 - t1, 3), "pack_cache": round(t3 - t2, 3), "total": round(t3 - t1, 3)}
    out["pack_episodes_device_s"] = round(t4 - t3, 3)
    out["rows"] = len(direct)
  line = json.dumps(out)
  print(line)
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  with open(a.out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()
