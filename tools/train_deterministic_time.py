"""ms per training step with the deterministic mode on and off: `DIMTrainer.train_step` at batch 128 and 512 and
`CILTrainer.train_step` (T = 4) at 512, the same synthetic observations, the two trainers of a configuration taking
turns region by region in one process.  Device events around `steps` train_step calls after `warmup` ones; the median
of `rounds` regions and their spread (min .. max) are reported.  One JSON line on stdout.

    python tools/train_deterministic_time.py [--steps 10] [--warmup 3] [--rounds 7]
    python tools/train_deterministic_time.py --default-only --root /path/to/another/checkout

`--default-only --root DIR` measures the default path of the package under DIR (e.g. the parent commit, which has no
`deterministic=` keyword) with the same regions: a job that alternates the two invocations puts the default path of two
commits side by side in one visit.

`--expect` prints, without a GPU, what the mode adds per step from the layer plan's shapes: the bytes of the partial
tables that are written and read back (the split rule is csrc/train.hip `gemm()`'s, restated here)."""
import argparse
import json
import os
import sys

import numpy as np


def split_of(ta, M, N, K):
  """csrc/train.hip gemm(): the number of K splits of a call (1 = not split)."""
  bn = 16 if (N <= 16 and M >= 256) else (32 if (N <= 32 and M >= 128) else 64)
  bm, bk = {16: (256, 16), 32: (128, 32), 64: (64, 32)}[bn]
  tiles = -(-N // bn) * -(-M // bm)
  if (K >= (1024 if ta else 4096) and tiles < 512) or (not ta and K >= 512 and tiles < 128):
    splits = min(-(-1024 // tiles), -(-K // 256))
    if splits > 1:
      kchunk = -(-(-(-K // splits)) // bk) * bk
      return -(-K // kchunk)
  return 1


def expected_partial_bytes(kind, B, T=4, C=2):
  """(bytes of partial tables written per training step, number of second-stage launches): every table is written once
  and read once, so the extra traffic of the mode is twice the first number (minus the atomics it replaces)."""
  from oatomobile_amd import arch
  calls = []  # (ta, M, N, K)

  def pointwise(rows, cin, cout):
    calls.extend([(False, rows, cout, cin), (True, cout, cin, rows), (False, rows, cin, cout)])

  dw = []  # (cout, h_out)
  for b in arch.blocks():
    if b.expand:
      pointwise(B * b.h_in**2, b.inp, b.hidden)
    dw.append((b.hidden, b.h_out))
    pointwise(B * b.h_out**2, b.hidden, b.oup)
  last_h = arch.blocks()[-1].h_out
  pointwise(B * last_h**2, arch.blocks()[-1].oup, arch.LAST_CHANNELS)
  nin = 128 + (5 if kind == "dim" else 6)
  calls += [(False, B, 128, 1280), (False, B, 64, nin), (False, B, 64, 64), (False, B, 64, 64)]  # head forward
  calls += [(True, 64, 64, B), (False, B, 64, 64)] * 2 + [(True, 64, nin, B), (False, B, nin, 64),
                                                          (True, 128, 1280, B), (False, B, 1280, 128)]
  R = B * T
  calls += [(True, 192, 2, R), (True, 192, 64, R)]
  calls += [(True, 32, 64, R), (True, 4, 32, R)] if kind == "dim" else [(True, 2, 64, R)]
  total, launches = 0, 0
  for ta, M, N, K in calls:
    s = split_of(ta, M, N, K)
    if s > 1:
      total += 4 * s * M * N
      launches += 1
  M0 = B * 50 * 50  # stem_wgrad: blocks x 32 x C x 9
  total += 4 * -(-M0 // max(512, -(-M0 // 512))) * 32 * C * 9
  launches += 1
  for cout, h in dw:  # dw_wgrad: grid.y x cout x 9 (encoder_backward's launch shape)
    chunks = (cout // 4 + 15) // 16
    G = max(1, min(8, B * chunks // 512))
    groups = -(-B // G)
    bands = max(1, min(h // 4, 1024 // (groups * chunks)))
    total += 4 * groups * bands * cout * 9
    launches += 1
  return total, launches


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--default-only", action="store_true")
  ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  ap.add_argument("--expect", action="store_true")
  a = ap.parse_args()
  sys.path.insert(0, os.path.abspath(a.root))
  configs = [("dim", 128), ("dim", 512), ("cil", 512)]
  if a.expect:
    out = {}
    for kind, B in configs:
      nbytes, launches = expected_partial_bytes(kind, B)
      out["%s_b%d" % (kind, B)] = {"partial_table_MB_per_step": round(nbytes / 1e6, 2), "second_stage_launches": launches}
    print(json.dumps(out))
    return
  import torch
  from oatomobile_amd import BehaviouralModel, CILTrainer, DIMTrainer, ImitativeModel, transform_visual
  if not torch.cuda.is_available():
    raise SystemExit("train_deterministic_time.py needs a GPU")
  dev = torch.device("cuda", 0)
  rng = np.random.default_rng(77)
  Bmax = max(B for _, B in configs)
  lidar = ((rng.integers(0, 6, size=(Bmax, 200, 200, 2)) / 5.0) * (rng.random((Bmax, 200, 200, 2)) < 0.12)).astype(np.float32)
  ctx = dict(visual_features=transform_visual(torch.from_numpy(lidar).to(dev), channels_last=True),
             velocity=torch.from_numpy(rng.normal(0, 3.0, size=(Bmax, 3)).astype(np.float32)).to(dev),
             is_at_traffic_light=torch.from_numpy((rng.random((Bmax, 1)) < 0.2).astype(np.float32)).to(dev),
             traffic_light_state=torch.from_numpy(rng.integers(0, 4, size=(Bmax, 1)).astype(np.float32)).to(dev),
             mode=torch.from_numpy(rng.choice([0.0, 2.0, 3.0], size=(Bmax, 1)).astype(np.float32)).to(dev),
             player_future=torch.from_numpy(np.cumsum(np.abs(rng.normal(size=(Bmax, 4, 3))) * 0.5, axis=1).astype(np.float32)).to(dev))
  out = {"steps_per_region": a.steps, "regions": a.rounds, "root": os.path.abspath(a.root), "device": torch.cuda.get_device_name(0)}
  for kind, B in configs:
    batch = {k: v[:B].contiguous() for k, v in ctx.items() if kind == "cil" or k != "mode"}
    modes = {"default": {}} if a.default_only else {"default": {}, "deterministic": {"deterministic": True}}
    trainers = {}
    for name, kw in modes.items():
      if kind == "dim":
        trainers[name] = DIMTrainer(ImitativeModel.synthetic(7, max_batch=1).to(dev), lr=1e-3, max_batch=B, device=dev, **kw)
      else:
        trainers[name] = CILTrainer(BehaviouralModel.synthetic(7, output_shape=(4, 2)).to(dev), lr=1e-3, max_batch=B,
                                    device=dev, **kw)
    for tr in trainers.values():
      for _ in range(a.warmup):
        tr.train_step(batch)
    torch.cuda.synchronize()
    times = {name: [] for name in trainers}
    for _ in range(a.rounds):
      for name, tr in trainers.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
          tr.train_step(batch)
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) / a.steps)
    rec = {}
    for name, ts in times.items():
      rec[name + "_ms_per_step"] = round(float(np.median(ts)), 4)
      rec[name + "_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
    if "deterministic" in times:
      rec["deterministic_over_default"] = round(rec["deterministic_ms_per_step"] / rec["default_ms_per_step"], 4)
      nbytes, launches = expected_partial_bytes(kind, B)
      rec["partial_table_MB_per_step"] = round(nbytes / 1e6, 2)
      rec["second_stage_launches"] = launches
    out["%s_b%d" % (kind, B)] = rec
    for tr in trainers.values():
      tr.close()
    del trainers
    torch.cuda.empty_cache()
  print(json.dumps(out))


if __name__ == "__main__":
  main()
