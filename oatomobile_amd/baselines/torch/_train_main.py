"""The command-line training of `python -m oatomobile_amd.baselines.torch.{dim,cil}.train`: the reference's `main()`
(oatomobile/baselines/torch/dim/train.py:85-322, cil/train.py:84-287) on this package's pieces.

    datum files (<dataset_dir>/{train,val}/*.npz) -> replay.pack_cache(targets=True) under --cache_dir (reused while
    its sources.json matches the datum files; with --raw_dataset: raw episodes -> replay.pack_episodes) -> replay.DeviceCache -> DIMTrainer / CILTrainer.train_epoch (batches assembled on the GPU) and
    evaluate_epoch at 5x the batch -> <output_dir>/ckpts/model-{epoch}.pt every --save_model_frequency epochs
    (Checkpointer.save: torch.save(model.state_dict())) and <output_dir>/logs/metrics.jsonl.

Flags keep the reference's names and defaults (argparse: absl is not a dependency here).  The initial weights are this
package's seeded synthetic initialisation (`ImitativeModel.synthetic` / `BehaviouralModel.synthetic`, --seed), not
torch's default initialisers.  TensorBoard logging and the prediction images of the reference's `write()` are not
reproduced; metrics.jsonl holds one line per epoch and split."""

import argparse
import glob
import json
import os
import time

import torch

NOISE_LEVEL = 1e-2  # dim/train.py:100


def parse_args(kind: str, argv=None) -> argparse.Namespace:
  p = argparse.ArgumentParser(prog="python -m oatomobile_amd.baselines.torch.%s.train" % kind,
                              description="Trains the %s model on expert demonstrations (MI355X)." %
                              {"dim": "deep imitative", "cil": "behavioural cloning"}[kind])
  p.add_argument("--dataset_dir", required=True, help="The full path to the processed dataset (train/ and val/).")
  p.add_argument("--output_dir", required=True, help="The full path to the output directory (for logs, ckpts).")
  p.add_argument("--batch_size", type=int, default=512, help="The batch size used for training the neural network.")
  p.add_argument("--num_epochs", type=int, required=True, help="The number of training epochs for the neural network.")
  p.add_argument("--save_model_frequency", type=int, default=4, help="The number epochs between saves of the model.")
  p.add_argument("--learning_rate", type=float, default=1e-3, help="The ADAM learning rate.")
  p.add_argument("--num_timesteps_to_keep", type=int, default=4,
                 help="The numbers of time-steps to keep from the target, with downsampling.")
  p.add_argument("--weight_decay", type=float, default=0.0, help="The L2 penalty (regularization) coefficient.")
  p.add_argument("--clip_gradients", action="store_true", default=False,
                 help="If True it clips the gradients norm to 1.0.")
  p.add_argument("--cache_dir", default=None, help="Packed caches of train/ and val/ (default <output_dir>/cache); "
                 "reused while they match the datum files.")
  p.add_argument("--raw_dataset", action="store_true", default=False,
                 help="<dataset_dir>/{train,val} hold RAW episodes (<episode>/<sample>.npz + metadata), not processed "
                 "datums: they are labelled in hindsight and packed in one step (replay.pack_episodes, the defaults of "
                 "CARLADataset.process: future 80, past 20, every 5th frame).")
  p.add_argument("--seed", type=int, default=0, help="Seeds the initial weights and the epoch generator.")
  p.add_argument("--deterministic", action="store_true", default=False,
                 help="Fixed-order sums in the training step: the same --seed, data, batch size and device model give "
                 "the same bits on every run (a little slower; DESIGN.md section 4.3g).")
  args = p.parse_args(argv)
  if kind == "dim" and args.num_timesteps_to_keep != 4:
    p.error("the DIM model is built for num_timesteps_to_keep=4 only (ImitativeModel(output_shape=(4, 2))); got %d" %
            args.num_timesteps_to_keep)
  if args.batch_size < 1 or args.num_epochs < 0 or args.save_model_frequency < 1:
    p.error("--batch_size and --save_model_frequency must be >= 1, --num_epochs >= 0")
  return args


SOURCES = "sources.json"  # beside the packed cache: the datum files it was packed from


def _sources(files):
  """What identifies the datum files a pack was made from: name, size and modification time of each, in order."""
  out = []
  for f in files:
    st = os.stat(f)
    out.append([os.path.basename(f), st.st_size, st.st_mtime_ns])
  return out


def packed(split_dir: str, cache_dir: str, raw: bool = False, device=None):
  """The packed cache of the datums in `split_dir`, packed once into `cache_dir`.  It is reused only when it has the
  training targets and `sources.json` lists the same datum files (name, size, modification time); a changed, added or
  removed file repacks it.  `raw`: `split_dir` holds raw episodes, packed with `replay.pack_episodes` (labelled on
  `device`, None = numpy); `sources.json` then lists the raw sample files of every episode."""
  from oatomobile_amd import replay
  if raw:
    files = sorted(glob.glob(os.path.join(split_dir, "*", "*.npz")))
    if not files:
      raise SystemExit("no raw episodes (<episode>/*.npz) under %s" % split_dir)
  else:
    files = sorted(glob.glob(os.path.join(split_dir, "*.npz")))  # replay.as_torch's order
    if not files:
      raise SystemExit("no datum files (*.npz) under %s" % split_dir)
  sources = _sources(files)
  try:
    with open(os.path.join(cache_dir, SOURCES)) as f:
      recorded = json.load(f)
    cache = replay.PackedCache(cache_dir)
    if cache.has_targets and (raw or len(cache) == len(files)) and recorded == sources:
      return cache
  except (OSError, ValueError):
    pass
  try:  # a pack interrupted or replaced below must not pass for the old one
    os.remove(os.path.join(cache_dir, SOURCES))
  except OSError:
    pass
  cache = replay.pack_episodes(split_dir, cache_dir, device=device) if raw else replay.pack_cache(files, cache_dir, targets=True)
  with open(os.path.join(cache_dir, SOURCES), "w") as f:
    json.dump(sources, f)
  return cache


def nll_limit(T: int) -> float:
  """dim/train.py:167-173: the NLL of the N(0, noise_level^2) perturbation itself, the theoretical minimum."""
  d = T * 2
  dist = torch.distributions.MultivariateNormal(loc=torch.zeros(d), scale_tril=torch.eye(d) * NOISE_LEVEL)
  return float(-torch.sum(dist.log_prob(torch.zeros(d))))


def main(kind: str, argv=None) -> int:
  from oatomobile_amd import replay
  from oatomobile_amd.cil import BehaviouralModel
  from oatomobile_amd.model import ImitativeModel
  from oatomobile_amd.train import CILTrainer, DIMTrainer
  args = parse_args(kind, argv)
  if not torch.cuda.is_available():
    raise SystemExit("oatomobile_amd trains on a ROCm device; none is visible")
  device = torch.device("cuda", torch.cuda.current_device())
  log_dir = os.path.join(args.output_dir, "logs")
  ckpt_dir = os.path.join(args.output_dir, "ckpts")
  for d in (args.output_dir, log_dir, ckpt_dir):
    os.makedirs(d, exist_ok=True)
  cache_dir = args.cache_dir or os.path.join(args.output_dir, "cache")
  caches = {split: packed(os.path.join(args.dataset_dir, split), os.path.join(cache_dir, split), args.raw_dataset,
                          device if args.raw_dataset else None) for split in ("train", "val")}
  C = caches["train"].channels
  data = {split: replay.DeviceCache(c, device) for split, c in caches.items()}
  T = args.num_timesteps_to_keep
  replay.downsample_stride(data["train"].L, T)  # the target slice must give T steps (ValueError otherwise)
  # the validation batch is 5x the training batch (dim/train.py:160, cil/train.py:156), evaluated in chunks of max_batch
  if kind == "dim":
    model = ImitativeModel.synthetic(args.seed, in_channels=C).to(device)
    trainer = DIMTrainer(model, lr=args.learning_rate, weight_decay=args.weight_decay, noise_level=NOISE_LEVEL,
                         max_batch=args.batch_size, device=device, deterministic=args.deterministic)
  else:
    model = BehaviouralModel.synthetic(args.seed, in_channels=C, output_shape=(T, 2)).to(device)
    trainer = CILTrainer(model, lr=args.learning_rate, weight_decay=args.weight_decay, max_batch=args.batch_size,
                         device=device, deterministic=args.deterministic)
  gen = torch.Generator(device=device).manual_seed(args.seed)
  extra = {"nll_limit": nll_limit(T)} if kind == "dim" else {}
  with open(os.path.join(log_dir, "metrics.jsonl"), "a") as log:
    for epoch in range(args.num_epochs):
      losses = {}
      for split in ("train", "val"):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        if split == "train":
          loss = trainer.train_epoch(data[split], args.batch_size, generator=gen, clip=args.clip_gradients)
        else:
          loss = trainer.evaluate_epoch(data[split], args.batch_size * 5, generator=gen, shuffle=True)
        dt = time.perf_counter() - t0  # the epoch's one .item() has synchronised
        losses[split] = loss
        line = dict(epoch=epoch, split=split, loss=loss, observations=len(data[split]),
                    observations_per_s=len(data[split]) / dt, seconds=dt, **extra)
        log.write(json.dumps(line) + "\n")
        log.flush()
      if epoch % args.save_model_frequency == 0:  # Checkpointer.save (torch/savers.py:37-42)
        torch.save({k: v.cpu() for k, v in trainer.state_dict().items()}, os.path.join(ckpt_dir, "model-%d.pt" % epoch))
      tail = " | THEORYMIN: %.2f" % extra["nll_limit"] if extra else ""
      print("epoch %d | TL: %.4f | VL: %.4f%s" % (epoch, losses["train"], losses["val"], tail), flush=True)
  trainer.sync_to_model()
  return 0
