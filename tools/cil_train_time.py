"""ms per training step: CILTrainer (cil/train.py:168-190) at T = 4 (the reference's training horizon) and T = 40
(CILAgent's) next to DIMTrainer, same batch (default 512, the CIL script's default), same synthetic observations.
Device events around `steps` train_step calls after `warmup` ones; the three trainers take turns for `rounds` rounds
(the median round is reported).  One JSON line on stdout.

    python tools/cil_train_time.py [--batch 512] [--steps 10] [--warmup 2] [--rounds 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=512)
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--rounds", type=int, default=3)
  a = ap.parse_args()
  from oatomobile_amd import BehaviouralModel, CILTrainer, DIMTrainer, ImitativeModel, transform_visual
  from tests.helpers import synth_observation
  if not torch.cuda.is_available():
    raise SystemExit("cil_train_time.py needs a GPU")
  dev = torch.device("cuda", 0)
  B = a.batch
  rng = np.random.default_rng(77)
  obs = [synth_observation(rng) for _ in range(B)]
  ctx = dict(visual_features=transform_visual(torch.from_numpy(np.stack([o["lidar"] for o in obs])).to(dev), channels_last=True),
             velocity=torch.from_numpy(np.stack([o["velocity"] for o in obs])).to(dev),
             is_at_traffic_light=torch.tensor([[float(o["is_at_traffic_light"])] for o in obs], device=dev),
             traffic_light_state=torch.tensor([[float(o["traffic_light_state"])] for o in obs], device=dev),
             mode=torch.from_numpy(rng.choice([0.0, 2.0, 3.0], size=(B, 1)).astype(np.float32)).to(dev))

  def future(T):
    return torch.from_numpy(np.cumsum(np.abs(rng.normal(size=(B, T, 3))) * 0.5, axis=1).astype(np.float32)).to(dev)

  runs = {
      "dim": (DIMTrainer(ImitativeModel.synthetic(7, max_batch=1).to(dev), lr=1e-3, max_batch=B, device=dev),
              dict(ctx, player_future=future(4))),
      "cil_T4": (CILTrainer(BehaviouralModel.synthetic(7, output_shape=(4, 2)).to(dev), lr=1e-3, max_batch=B, device=dev),
                 dict(ctx, player_future=future(4))),
      "cil_T40": (CILTrainer(BehaviouralModel.synthetic(7, output_shape=(40, 2)).to(dev), lr=1e-3, max_batch=B, device=dev),
                  dict(ctx, player_future=future(40))),
  }
  for tr, batch in runs.values():
    for _ in range(a.warmup):
      tr.train_step(batch)
  torch.cuda.synchronize()
  times = {k: [] for k in runs}
  losses = {k: [] for k in runs}
  for _ in range(a.rounds):
    for name, (tr, batch) in runs.items():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(a.steps):
        losses[name].append(tr.train_step(batch))
      e1.record()
      torch.cuda.synchronize()
      times[name].append(e0.elapsed_time(e1) / a.steps)
  out = {"batch": B, "steps_per_round": a.steps, "rounds": a.rounds}
  for name in runs:
    out[name + "_ms_per_step"] = float(np.median(times[name]))
    out[name + "_ms_rounds"] = [round(x, 3) for x in times[name]]
    l = [float(x) for x in losses[name]]
    out[name + "_loss_first_last"] = [l[0], l[-1]]
  out["cil_T4_over_dim"] = out["cil_T4_ms_per_step"] / out["dim_ms_per_step"]
  out["cil_T40_over_dim"] = out["cil_T40_ms_per_step"] / out["dim_ms_per_step"]
  print(json.dumps(out))


if __name__ == "__main__":
  main()
