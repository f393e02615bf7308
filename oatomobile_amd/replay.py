"""Offline replay of cached observations (BASELINE config 5).

Reads the reference's on-disk formats —
  * datum files: one compressed `.npz` per frame with the sensor keys (`lidar`, `velocity`,
    `is_at_traffic_light`, `traffic_light_state`, `player_future`, ...), loaded like
    `CARLADataset.load_datum` (oatomobile/datasets/carla.py:107-164);
  * episodes: `<parent>/<token>/<sample>.npz` + a `metadata` file listing sample tokens in order
    (oatomobile/core/dataset.py:32-109)
— and pushes them through `RIPAgent.plan_batch` in device-resident batches (observation-parallel: with several
ranks each replays `distributed.shard_range(len(files), rank, world)`).

`goal` is not among the collected sensors (datasets/carla.py:175-182); like SURVEY §8d config 5 it is derived
from the recorded future: every `stride`-th waypoint of `player_future`, first `num_goals`, xy only.
"""

import io
import os
import uuid
from typing import List, Mapping, Optional, Sequence

import numpy as np
import torch

from oatomobile_amd._datum import MODALITIES, _fill_rows, goal_from_future, load_datum  # noqa: F401  (torch-free)


class Episode:
  """core/dataset.py:32-109: a directory of `.npz` samples + `metadata` token list."""

  def __init__(self, parent_dir: str, token: str) -> None:
    self._parent_dir, self._token = parent_dir, token
    self._episode_dir = os.path.join(parent_dir, token)
    os.makedirs(self._episode_dir, exist_ok=True)  # core/dataset.py:46-48
    self._metadata_fname = os.path.join(self._episode_dir, "metadata")

  def append(self, *sample_token: str, **observations: np.ndarray) -> None:
    """core/dataset.py:53-70: one compressed `.npz` per sample under a fresh random token (uuid4 hex, like
    utils/uuid.py); an explicit token may be passed positionally (deterministic tests)."""
    if len(sample_token) > 1:
      raise TypeError("append() takes at most one positional argument (the sample token)")
    token = sample_token[0] if sample_token else uuid.uuid4().hex
    np.savez_compressed(os.path.join(self._episode_dir, "%s.npz" % token), **observations)
    with open(self._metadata_fname, "a") as f:
      f.write("%s\n" % token)

  def read_sample(self, sample_token: str, attr: Optional[str] = None):
    """core/dataset.py:79-109: the whole observation of a sample, or one attribute of it."""
    with np.load(self.sample_path(sample_token), allow_pickle=True) as npz_file:
      if attr is not None:
        return npz_file[attr]
      return {k: npz_file[k] for k in npz_file}

  def fetch(self) -> List[str]:
    with open(self._metadata_fname) as f:
      return [t for t in f.read().split("\n") if t]

  def sample_path(self, sample_token: str) -> str:
    return os.path.join(self._episode_dir, "%s.npz" % sample_token)

  def files(self) -> List[str]:
    return [self.sample_path(t) for t in self.fetch()]


def as_torch(dataset_dir: str, modalities: Sequence[str] = MODALITIES, transform=None, mode: bool = False,
             only_array: bool = False) -> "torch.utils.data.Dataset":
  """`CARLADataset.as_torch` (datasets/carla.py:617-695): the unbatched map-style dataset over `<dataset_dir>/*.npz` —
  every item is `load_datum(..., dataformat="CHW")` without its non-array entries (`name`), with `transform` applied to
  each value.  Files are taken in sorted order (the reference keeps `glob`'s).  `only_array` is accepted for signature
  parity; the reference filters the non-array keys regardless of it."""
  import glob
  del only_array

  class _Datums(torch.utils.data.Dataset):

    def __init__(self):
      self._npz_files = sorted(glob.glob(os.path.join(dataset_dir, "*.npz")))

    def __len__(self) -> int:
      return len(self._npz_files)

    def __getitem__(self, idx: int):
      sample = load_datum(self._npz_files[idx], modalities=modalities, mode=mode, dataformat="CHW")
      sample = {k: v for k, v in sample.items() if isinstance(v, np.ndarray)}
      if transform is not None:
        sample = {k: transform(v) for k, v in sample.items()}
      return sample

  return _Datums()


def effective_cpus() -> int:
  """CPUs this process may actually use: the affinity mask capped by the cgroup CPU quota (containers report the
  host's core count in `os.cpu_count()`; worker processes beyond the quota are throttled and slow everything down:
  measured on the bench host, quota 16 of 256 threads: 16 decode processes 5.9 k datums/s, 64 processes 1.4 k)."""
  n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
  try:
    with open("/sys/fs/cgroup/cpu.max") as f:  # cgroup v2: "<quota> <period>" or "max <period>"
      quota, period = f.read().split()
    if quota != "max":
      n = min(n, max(1, int(int(quota) / int(period))))
  except (OSError, ValueError):
    try:
      with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
        quota = int(f.read())
      with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
        period = int(f.read())
      if quota > 0:
        n = min(n, max(1, quota // period))
    except (OSError, ValueError):
      pass
  return n


def _decode_worker(w, nworkers, files, batch_size, names, ctrl_name, shapes, ring, num_goals, goal_stride):
  """Worker process of `DatumBatches`: decodes rows [w * per, (w + 1) * per) of EVERY batch straight into the batch's
  shared-memory buffer.  No task queue: the schedule is static, the only traffic with the parent is two flags in a
  shared control block (`consumed` batches, written by the parent; `done[w, b]`, written by this worker)."""
  import time
  from multiprocessing import shared_memory
  blocks = [[shared_memory.SharedMemory(name=n) for n in slot] for slot in names]
  bufs = [[np.ndarray(s, np.float32, buffer=b.buf) for s, b in zip(shapes, slot)] for slot in blocks]
  ctrl = shared_memory.SharedMemory(name=ctrl_name)
  nb = (len(files) + batch_size - 1) // batch_size
  head = np.ndarray((2,), np.int64, buffer=ctrl.buf)                       # [consumed, stop]
  done = np.ndarray((nworkers, nb), np.uint8, buffer=ctrl.buf, offset=16)
  try:
    for b in range(nb):
      while b >= head[0] + ring and not head[1]:
        time.sleep(2e-4)
      if head[1]:
        break
      chunk = files[b * batch_size:(b + 1) * batch_size]
      per = (len(chunk) + nworkers - 1) // nworkers
      j0 = w * per
      if j0 < len(chunk):
        lidar, vec, goal = bufs[b % ring]
        _fill_rows(chunk[j0:j0 + per], j0, lidar, vec, goal, num_goals, goal_stride)
      done[w, b] = 1
  finally:
    del head, done, bufs
    for slot in blocks:
      for blk in slot:
        blk.close()
    ctrl.close()


class DatumBatches:
  """Host batches `(lidar [n,H,W,C], vec [n,5], goal [n,G,2])` (float32 torch tensors) over a list of datum files.

  `workers == 0`: decoded inline into pinned staging buffers.  `workers > 0`: the reference's answer to the decode
  cost — worker PROCESSES (`dim/train.py:150-155` gives its DataLoader 50) — with two differences: a worker writes its
  rows of a batch straight into a shared-memory batch buffer (nothing is pickled or collated), and the schedule is
  static (worker w owns the w-th slice of every batch), so there is no task queue: on the 256-thread bench host a
  `multiprocessing.Pool` spent 60 ms per task in dispatch, more than the decode itself.  `prefetch` batches are decoded
  ahead of the one being consumed.  The tensors of a batch are views of its buffer: use (upload) them before asking
  for the next batch."""

  def __init__(self, files: Sequence[str], batch_size: int, num_goals: int = 10, goal_stride: int = 8, workers: int = 0,
               prefetch: int = 2, channels: Optional[int] = None) -> None:
    self._files, self._bs = list(files), int(batch_size)
    self._ng, self._gs = int(num_goals), int(goal_stride)
    self._workers, self._prefetch = int(workers), max(1, int(prefetch))
    self._procs, self._shm, self._registered = [], [], []
    if not self._files:
      self._shapes = None
      return
    H, W, C = load_datum(self._files[0], modalities=("lidar",))["lidar"].shape
    if channels is not None and C != channels:
      raise ValueError("datums have %d BEV channels, the agent expects %d" % (C, channels))
    self._shapes = ((self._bs, H, W, C), (self._bs, 5), (self._bs, self._ng, 2))

  def __len__(self) -> int:
    return (len(self._files) + self._bs - 1) // self._bs

  def close(self) -> None:
    for p in self._procs:
      p.join(timeout=5)
      if p.is_alive():
        p.terminate()
    self._procs = []
    if self._registered:
      rt = torch.cuda.cudart()
      for ptr in self._registered:
        try:
          rt.cudaHostUnregister(ptr)
        except Exception:
          pass
      self._registered = []
    for b in self._shm:
      try:
        b.close()
        b.unlink()
      except (FileNotFoundError, BufferError):
        pass
    self._shm = []

  def __iter__(self):
    if not self._files:
      return
    nb = len(self)
    slots = None
    if self._workers > 0:
      from multiprocessing import shared_memory
      ring = self._prefetch + 1
      try:
        slots = []
        for _ in range(ring):
          slot = []
          slots.append(slot)
          for shp in self._shapes:
            slot.append(shared_memory.SharedMemory(create=True, size=int(np.prod(shp)) * 4))
      except OSError as exc:  # /dev/shm too small for the batch ring: decode inline instead of failing the replay
        import warnings
        for slot in slots or []:
          for blk in slot:
            blk.close()
            blk.unlink()
        slots = None
        warnings.warn("DatumBatches: no shared memory for %d batch buffers (%s); decoding in this process" % (ring, exc))
    if slots is None:
      pinned = torch.cuda.is_available()
      arrs = [torch.empty(s).pin_memory() if pinned else torch.empty(s) for s in self._shapes]
      views = [a.numpy() for a in arrs]
      for b in range(nb):
        n = _fill_rows(self._files[b * self._bs:(b + 1) * self._bs], 0, views[0], views[1], views[2], self._ng, self._gs)
        yield tuple(a[:n] for a in arrs)
      return
    import multiprocessing as mp
    import time
    nw = min(self._workers, self._bs)
    head = done = None
    self._shm = [b for slot in slots for b in slot]
    try:
      ctrl = shared_memory.SharedMemory(create=True, size=16 + nw * nb)
      self._shm = [b for slot in slots for b in slot] + [ctrl]
      head = np.ndarray((2,), np.int64, buffer=ctrl.buf)
      done = np.ndarray((nw, nb), np.uint8, buffer=ctrl.buf, offset=16)
      head[:] = 0
      done[:] = 0
      views = [[np.ndarray(s, np.float32, buffer=b.buf) for s, b in zip(self._shapes, slot)] for slot in slots]
      names = [[b.name for b in slot] for slot in slots]
      # page-lock the batch buffers for the device (hipHostRegister): the upload of a batch is then one DMA at PCIe
      # rate (3 ms per 164 MB) instead of a staged pageable copy (35 ms of a host core)
      if torch.cuda.is_available():
        try:
          rt = torch.cuda.cudart()
          for slot in slots:
            for blk, shape in zip(slot, self._shapes):
              arr = np.ndarray(shape, np.float32, buffer=blk.buf)
              if int(rt.cudaHostRegister(arr.ctypes.data, arr.nbytes, 0)) == 0:
                self._registered.append(arr.ctypes.data)
              del arr
        except Exception:  # registration is an optimisation only
          pass
      ctx = mp.get_context("spawn")  # the parent usually holds a HIP context, which a forked child must not inherit
      self._procs = [ctx.Process(target=_decode_worker, daemon=True,
                                 args=(w, nw, self._files, self._bs, names, ctrl.name, self._shapes, ring, self._ng, self._gs))
                     for w in range(nw)]
      for p in self._procs:
        p.start()
      for b in range(nb):
        while not done[:, b].all():
          if any(p.exitcode not in (None, 0) for p in self._procs):
            raise RuntimeError("a datum decode worker died (exit codes %s)" % [p.exitcode for p in self._procs])
          time.sleep(2e-4)
        n = min(self._bs, len(self._files) - b * self._bs)
        yield tuple(torch.from_numpy(v[:n]) for v in views[b % ring])
        head[0] = b + 1  # the consumer is done with batch b: its buffer may be refilled
    finally:
      if head is not None:
        head[1] = 1
      del head, done
      views = None
      self.close()


def replay(agent, files: Sequence[str], batch_size: int, num_goals: int = 10, goal_stride: int = 8,
           workers: Optional[int] = 0, interpolate: bool = False) -> np.ndarray:
  """Plans for every datum in `files` -> [len(files), 4, 2] float32 (host), or with `interpolate=True` what
  `agent(observation)` returns per datum: [len(files), 30, 3] float64 (rip/agent.py:141-151, computed on the device).
  `agent` is a `RIPAgent` built with `max_batch >= batch_size`.

  Decode (np.load: zipfile + zlib + dtype conversion, ~0.7 ms per 200x200x2 frame, under the GIL) bounds this loop:
  1.4 k observations/s inline against 70 k/s of act() on the device, and a thread pool is slower still.
  `workers = W` decodes in W processes (`DatumBatches`; None = `effective_cpus() - 1`) while the device works on the
  previous batch; sharding `files` over ranks (`distributed.shard_range`) multiplies that."""
  dev = agent._device
  out = np.empty((len(files), 30, 3), np.float64) if interpolate else np.empty((len(files), 4, 2), np.float32)
  if len(files) == 0:
    return out
  if workers is None:  # everything the process may use, one CPU left to the parent
    workers = max(1, min(48, effective_cpus() - 1))
  i0 = 0
  for lidar, vec, goal in DatumBatches(files, batch_size, num_goals, goal_stride, workers, channels=agent._in_channels):
    n = lidar.shape[0]
    plan = agent.plan_batch(lidar.to(dev, non_blocking=True), vec.to(dev, non_blocking=True),
                            goal.to(dev, non_blocking=True), interpolate=interpolate)
    out[i0:i0 + n] = plan.cpu().numpy()
    i0 += n
  return out


# ---------------------------------------------------------------------------------------------------------
# Packed replay cache: one-time conversion of the `.npz` datums, decode-free replay afterwards
# ---------------------------------------------------------------------------------------------------------
CACHE_FILES = ("codes.npy", "lut.npy", "vec.npy", "goal.npy")


def pack_cache(files: Sequence[str], out_dir: str, num_goals: int = 10, goal_stride: int = 8, channels: Optional[int] = None,
               chunk: int = 256, workers: Optional[int] = None, targets: bool = False) -> "PackedCache":
  """One-time conversion of datum files (the reference's compressed `.npz`, datasets/carla.py:107-164 — they stay the
  source of truth) into a packed cache under `out_dir`:

    codes.npy [n,H,W,C] uint8   the BEV, every cell an index into
    lut.npy   [256]    float32  the distinct float32 BIT PATTERNS `load_datum` yields for `lidar` over the whole file
                                list, in ascending order of the pattern read as uint32 (= ascending value for the
                                non-negative levels k/5 of the CARLA histogram, utils/carla.py:225-233; -0.0 is a value
                                of its own, after the positive ones), padded with NaN
    vec.npy   [n,5]    float32  velocity[3], is_at_traffic_light, traffic_light_state
    goal.npy  [n,G,2]  float32  `goal_from_future(player_future)`

  `targets=True` adds the training targets (`DeviceCache`, `_PackedTrainer.train_epoch`):

    future.npy [n,L,2] float32  `player_future[:, :2]` (L = 80 for the reference's `process()`)
    mode.npy   [n]     float32  the label `load_datum(mode=True)` gives (datasets/carla.py:148-162), as the datum says:
                                the CIL model's STOP -> FORWARD rewrite is applied when a batch is gathered

  `lut[codes]` reproduces `load_datum(...)["lidar"]` bit for bit — compared as uint32 patterns per chunk while packing,
  so the sign of a zero survives; more than 256 distinct values or a NaN raise ValueError: such data is not a clipped
  histogram and keeps the `.npz` path.  80 KB instead of 320 KB per 200 x 200 x 2 observation, read back with
  `np.load(mmap_mode="r")`: no zip, no zlib, no dtype conversion.

  Packing is embarrassingly parallel: `workers` processes (None = `effective_cpus()`, 0 / 1 = this process) each decode
  and code a contiguous span of the files straight into the `codes.npy` memmap against their own value table; this
  process unifies the tables and re-codes the (rare) chunks packed before a value was first seen.  The workers run
  `_datum.py` as a script: numpy only, no torch import, no inherited HIP context."""
  from oatomobile_amd import _datum
  n = len(files)
  if n == 0:
    raise ValueError("pack_cache: no files")
  files = [str(f) for f in files]
  os.makedirs(out_dir, exist_ok=True)
  first = load_datum(files[0])
  H, W, C = first["lidar"].shape
  L = int(first["player_future"].shape[0]) if targets else 0
  if channels is not None and C != channels:
    raise ValueError("pack_cache: datums have %d BEV channels, expected %d" % (C, channels))
  shape = (n, H, W, C)
  codes = np.lib.format.open_memmap(os.path.join(out_dir, "codes.npy"), mode="w+", dtype=np.uint8, shape=shape)
  del codes  # the spans open it themselves
  if workers is None:
    workers = effective_cpus()
  workers = max(1, min(int(workers), (n + chunk - 1) // chunk))
  vec = np.empty((n, 5), np.float32)
  goal = np.empty((n, num_goals, 2), np.float32)
  future = np.empty((n, L, 2), np.float32) if targets else None
  mode = np.empty((n,), np.float32) if targets else None
  spans = []  # (row0, rows, table the rows were coded against)
  if workers == 1:
    spans, vec, goal, future, mode = _datum.pack_span(files, 0, out_dir, shape, num_goals, goal_stride, chunk, L)
  else:
    import json
    import subprocess
    import sys
    import tempfile
    per = ((n + workers - 1) // workers + chunk - 1) // chunk * chunk  # whole chunks per worker
    with tempfile.TemporaryDirectory(prefix="rip_pack_") as tmp:
      jobs = []
      for w, i0 in enumerate(range(0, n, per)):
        job = dict(files=files[i0:i0 + per], i0=i0, out_dir=os.path.abspath(out_dir), shape=list(shape),
                   num_goals=num_goals, goal_stride=goal_stride, chunk=chunk, result=os.path.join(tmp, "r%d.npz" % w))
        if targets:
          job["future_len"] = L
        path = os.path.join(tmp, "j%d.json" % w)
        with open(path, "w") as fh:
          json.dump(job, fh)
        env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
        jobs.append((job, subprocess.Popen([sys.executable, os.path.abspath(_datum.__file__), path], env=env,
                                           stderr=subprocess.PIPE)))
      failure = None
      for job, proc in jobs:
        _, err = proc.communicate()
        if proc.returncode == 3 and failure is None:
          with open(job["result"] + ".err") as fh:
            failure = ValueError(fh.read())
        elif proc.returncode != 0 and failure is None:
          failure = RuntimeError("pack_cache: a packing worker failed (exit code %d): %s" %
                                 (proc.returncode, err.decode(errors="replace")[-2000:]))
        if proc.returncode == 0:
          with np.load(job["result"]) as r:
            i0, m = job["i0"], len(job["files"])
            vec[i0:i0 + m], goal[i0:i0 + m] = r["vec"], r["goal"]
            if targets:
              future[i0:i0 + m], mode[i0:i0 + m] = r["future"], r["mode"]
            off = 0
            for (row0, rows), size in zip(r["rows"], r["sizes"]):
              spans.append((int(row0), int(rows), r["tables"][off:off + int(size)].copy()))
              off += int(size)
      if failure is not None:
        raise failure
  return _write_cache(out_dir, spans, vec, goal, future if targets else None, mode if targets else None)


def _write_cache(out_dir: str, spans, vec, goal, future, mode) -> "PackedCache":
  """The end of a pack: unifies the value tables of `spans` [(row0, rows, table)], re-codes the rows of `codes.npy`
  that were coded against another table than the final one, and writes lut / vec / goal (/ future / mode) beside it."""
  targets = future is not None
  values = np.empty((0,), np.uint32)
  for _, _, t in spans:
    values = np.union1d(values, t).astype(np.uint32)
  if values.size > 256:
    raise ValueError("pack_cache: more than 256 distinct BEV values (%d): not a clipped histogram" % values.size)
  stale = [(r0, m, t) for r0, m, t in spans if not np.array_equal(t, values)]
  if stale:  # coded before a value was first seen (or in a span that never saw it): re-code against the final table
    codes = np.lib.format.open_memmap(os.path.join(out_dir, "codes.npy"), mode="r+")
    for r0, m, t in stale:
      remap = np.searchsorted(values, t).astype(np.uint8)
      codes[r0:r0 + m] = remap[codes[r0:r0 + m]]
    codes.flush()
    del codes
  lut = np.full((256,), np.nan, np.float32)
  lut[:values.size] = values.view(np.float32)
  np.save(os.path.join(out_dir, "lut.npy"), lut)
  np.save(os.path.join(out_dir, "vec.npy"), vec)
  np.save(os.path.join(out_dir, "goal.npy"), goal)
  if targets:
    np.save(os.path.join(out_dir, "future.npy"), future)
    np.save(os.path.join(out_dir, "mode.npy"), mode)
  return PackedCache(out_dir)


class PackedCache:
  """A cache written by `pack_cache`, memory-mapped: `len()`, `lidar(i)` (the float32 BEV `load_datum` would give),
  and `batches(batch_size)` -> host tensors `(codes [n,H,W,C] uint8, vec [n,5], goal [n,G,2])` in pinned staging
  buffers (two slots: the tensors of a batch stay valid while the next one is being filled).  A cache packed with
  `targets=True` also has `future` [n,L,2] and `mode` [n] (`has_targets`; both None otherwise)."""

  def __init__(self, cache_dir: str) -> None:
    self.dir = cache_dir
    self.codes = np.load(os.path.join(cache_dir, "codes.npy"), mmap_mode="r")
    self.lut = np.load(os.path.join(cache_dir, "lut.npy"))
    self.vec = np.load(os.path.join(cache_dir, "vec.npy"))
    self.goal = np.load(os.path.join(cache_dir, "goal.npy"))
    if not (self.codes.dtype == np.uint8 and self.codes.ndim == 4 and self.lut.shape == (256,) and
            self.vec.shape == (self.codes.shape[0], 5) and self.goal.shape[0] == self.codes.shape[0]):
      raise ValueError("%s is not a packed replay cache" % cache_dir)
    self.future = self.mode = None
    if os.path.exists(os.path.join(cache_dir, "future.npy")):
      self.future = np.load(os.path.join(cache_dir, "future.npy"), mmap_mode="r")
      self.mode = np.load(os.path.join(cache_dir, "mode.npy"), mmap_mode="r")
      if not (self.future.ndim == 3 and self.future.shape[0] == len(self) and self.future.shape[2] == 2 and
              self.mode.shape == (len(self),)):
        raise ValueError("%s: future.npy / mode.npy do not match the cache" % cache_dir)

  @property
  def has_targets(self) -> bool:
    return self.future is not None

  def __len__(self) -> int:
    return int(self.codes.shape[0])

  @property
  def channels(self) -> int:
    return int(self.codes.shape[3])

  def lidar(self, i: int) -> np.ndarray:
    return self.lut[np.asarray(self.codes[i])]

  def batches(self, batch_size: int, begin: int = 0, end: Optional[int] = None):
    end = len(self) if end is None else end
    n, H, W, C = self.codes.shape
    G = self.goal.shape[1]
    pin = torch.cuda.is_available()
    slots = [(torch.empty((batch_size, H, W, C), dtype=torch.uint8, pin_memory=pin),
              torch.empty((batch_size, 5), dtype=torch.float32, pin_memory=pin),
              torch.empty((batch_size, G, 2), dtype=torch.float32, pin_memory=pin)) for _ in range(2)]
    # the page-cache -> pinned copy of the codes is the only per-batch host work that scales with the batch (41 MB at
    # 512 observations): split over a few threads (numpy's copy releases the GIL)
    from concurrent.futures import ThreadPoolExecutor
    nthreads = max(1, min(4, effective_cpus() - 1))
    with ThreadPoolExecutor(nthreads) as pool:
      for k, i0 in enumerate(range(begin, end, batch_size)):
        m = min(batch_size, end - i0)
        c, v, g = slots[k & 1]
        cn = c.numpy()
        cuts = [m * t // nthreads for t in range(nthreads + 1)]
        list(pool.map(lambda ab: np.copyto(cn[ab[0]:ab[1]], self.codes[i0 + ab[0]:i0 + ab[1]]),
                      [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]))
        np.copyto(v.numpy()[:m], self.vec[i0:i0 + m])
        np.copyto(g.numpy()[:m], self.goal[i0:i0 + m])
        yield c[:m], v[:m], g[:m]


def _episodes(dataset_dir: str):
  """The episodes of a raw dataset in sorted order: every sub-directory with a `metadata` file
  (datasets/carla.py:260-268 skips the others) -> [(token, Episode, sample tokens in order)]."""
  out = []
  for token in sorted(os.listdir(dataset_dir)):
    if os.path.isfile(os.path.join(dataset_dir, token, "metadata")):
      episode = Episode(dataset_dir, token)
      out.append((token, episode, episode.fetch()))
  return out


def _cuda_device(device, what: str) -> torch.device:
  dev = torch.device(device)
  if dev.type != "cuda":
    raise RuntimeError("%s: device must be None (numpy) or a ROCm device, got %s" % (what, dev))
  return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _hindsight_launch(location, rotation, episode, frames, L, P, G, goal_stride, want):
  """One `rip_hindsight_targets` launch over device tensors -> dict of the outputs named in `want` (the others are
  passed as NULL).  No synchronisation."""
  from oatomobile_amd import _lib
  dev, M = location.device, int(frames.numel())
  spec = dict(future64=((M, L, 3), torch.float64), past64=((M, P, 3), torch.float64), future_xy=((M, L, 2), torch.float32),
              goal=((M, G, 2), torch.float32), mode=((M,), torch.float32), valid=((M,), torch.uint8))
  out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in spec.items() if k in want}
  arg = lambda k: _lib.ptr(out[k], spec[k][1]) if k in out else _lib.ptr(None)
  with torch.cuda.device(dev):  # stateless entry point: launches on the current device
    _lib.check(_lib.load().rip_hindsight_targets(
        _lib.ptr(location), _lib.ptr(rotation), _lib.ptr(episode, torch.int32), int(location.shape[0]),
        _lib.ptr(frames, torch.int32), M, int(L), int(P), int(G), int(goal_stride), arg("future64"), arg("past64"),
        arg("future_xy"), arg("goal"), arg("mode"), arg("valid"), _lib.current_stream(dev)))
  return out


def _episode_labels(name, episode, sequence, L, P, skips, device, want, G=1, goal_stride=1):
  """The poses of an episode, read once per sample, and the hindsight labels of its windows
  `range(P, len(sequence) - L, skips)` -> (frames, dict of host arrays): `_datum.hindsight_targets` for `device=None`,
  else one `rip_hindsight_targets` launch.  `want` names the outputs (future64, past64, future_xy, goal, mode)."""
  from oatomobile_amd import _datum
  if len(sequence) < P + L + 1:  # datasets/carla.py:271 asserts here
    raise ValueError("episode %s has %d samples, fewer than past_length + future_length + 1 = %d" %
                     (name, len(sequence), P + L + 1))
  location, rotation = [], []
  for token in sequence:  # one open per sample; only the two small members are decompressed
    with np.load(episode.sample_path(token), allow_pickle=True) as sample:
      location.append(np.asarray(sample["location"]).reshape(3))
      rotation.append(np.asarray(sample["rotation"]).reshape(3))
  location, rotation = np.stack(location), np.stack(rotation)
  frames = np.arange(P, len(sequence) - L, skips, dtype=np.int32)
  if device is None:
    future64, past64 = _datum.hindsight_targets(location, rotation, frames, L, P)
    out = dict(future64=future64, past64=past64)
    if {"future_xy", "goal", "mode"} & set(want):
      out["future_xy"], out["goal"], out["mode"] = _datum.targets_from_future(future64, G, goal_stride)
    return frames, {k: out[k] for k in want}
  if location.dtype != np.float32 or rotation.dtype != np.float32:
    raise ValueError("episode %s: the device path takes float32 poses (the sensors' dtype), got location %s, rotation %s; "
                     "use device=None" % (name, location.dtype, rotation.dtype))
  dev = _cuda_device(device, "hindsight labelling")
  up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
  out = _hindsight_launch(up(location), up(rotation), torch.zeros(len(sequence), dtype=torch.int32, device=dev), up(frames),
                          L, P, G, goal_stride, set(want) | {"valid"})
  host = {k: v.cpu().numpy() for k, v in out.items()}
  assert host.pop("valid").all()  # every window of range(P, n - L) is inside the episode
  return frames, host


def process(dataset_dir: str, output_dir: str, future_length: int = 80, past_length: int = 20, num_frame_skips: int = 5,
            device=None) -> List[str]:
  """`CARLADataset.process` (datasets/carla.py:237-325): raw episodes `<dataset_dir>/<episode>/<sample>.npz` ->
  one datum `<output_dir>/<sample>.npz` per window `i in range(past_length, len(sequence) - future_length,
  num_frame_skips)` of every episode (taken in sorted order): every key of the raw observation unchanged, plus
  `player_future` [L,3] and `player_past` [P,3] (float64), the locations of the next L and previous P samples in the
  sample's ego frame.  Returns the files written, in order.

  Differences: the reference opens L + P + 1 compressed files per datum; here the pose of every sample is read once per
  episode and the whole episode is labelled at once (`device=None`: numpy; a ROCm device: one `rip_hindsight_targets`
  launch).  The reference swallows every exception per datum (no file, no message); here an episode shorter than
  P + L + 1 samples is a ValueError that names it (the reference asserts) and any other error surfaces.  A directory
  without a `metadata` file is skipped, like there."""
  L, P, skips = int(future_length), int(past_length), int(num_frame_skips)
  if L < 1 or P < 0 or skips < 1:
    raise ValueError("process: future_length >= 1, past_length >= 0, num_frame_skips >= 1; got %d, %d, %d" % (L, P, skips))
  os.makedirs(output_dir, exist_ok=True)
  written = []
  for name, episode, sequence in _episodes(dataset_dir):
    frames, labels = _episode_labels(name, episode, sequence, L, P, skips, device, ("future64", "past64"))
    for m, i in enumerate(frames):
      observation = episode.read_sample(sequence[i])
      path = os.path.join(output_dir, "%s.npz" % sequence[i])
      np.savez_compressed(path, **observation, player_future=labels["future64"][m], player_past=labels["past64"][m])
      written.append(path)
  return written


def pack_episodes(dataset_dir: str, out_dir: str, future_length: int = 80, past_length: int = 20, num_frame_skips: int = 5,
                  num_goals: int = 10, goal_stride: int = 8, device=None, chunk: int = 256) -> "PackedCache":
  """Raw episodes straight to a packed cache with training targets: `pack_cache(files of process(...), targets=True)`
  without the datum files in between — rows in `process`'s order (episodes sorted, windows in sequence order), the same
  six files.  `codes.npy`, `lut.npy`, `vec.npy` and `mode.npy` equal that cache's bit for bit; `future.npy` and
  `goal.npy` equal it with `device=None` and are within one float32 ulp of it on a ROCm device (one
  `rip_hindsight_targets` launch per episode).  Every raw sample is decompressed once: its pose when its episode is
  labelled, its BEV only if it is a window's centre.  Packs in this process (`_datum.pack_span` with the labels handed
  over, then the table unification of `pack_cache`)."""
  from oatomobile_amd import _datum
  L, P, skips, G = int(future_length), int(past_length), int(num_frame_skips), int(num_goals)
  if L < 1 or P < 0 or skips < 1:
    raise ValueError("pack_episodes: future_length >= 1, past_length >= 0, num_frame_skips >= 1; got %d, %d, %d" % (L, P, skips))
  files, future, goal, mode = [], [], [], []
  for name, episode, sequence in _episodes(dataset_dir):
    frames, labels = _episode_labels(name, episode, sequence, L, P, skips, device, ("future_xy", "goal", "mode"), G,
                                     int(goal_stride))
    files += [episode.sample_path(sequence[i]) for i in frames]
    future.append(labels["future_xy"])
    goal.append(labels["goal"])
    mode.append(labels["mode"])
  if not files:
    raise ValueError("pack_episodes: no episodes under %s" % dataset_dir)
  os.makedirs(out_dir, exist_ok=True)
  H, W, C = load_datum(files[0], modalities=("lidar",))["lidar"].shape
  shape = (len(files), H, W, C)
  codes = np.lib.format.open_memmap(os.path.join(out_dir, "codes.npy"), mode="w+", dtype=np.uint8, shape=shape)
  del codes  # pack_span opens it itself
  labels = (np.concatenate(future), np.concatenate(goal), np.concatenate(mode))
  spans, vec, goal, future, mode = _datum.pack_span(files, 0, out_dir, shape, G, int(goal_stride), chunk, L, labels)
  return _write_cache(out_dir, spans, vec, goal, future, mode)


def downsample_stride(L: int, T: int) -> int:
  """transforms.downsample_target (torch/transforms.py:23-31) keeps `future[:, 0::L // T]`: that stride, or ValueError
  when the slice does not have exactly T steps (the reference would hand the model a target of another length)."""
  L, T = int(L), int(T)
  stride = L // T if T >= 1 else 0
  if stride < 1 or len(range(0, L, stride)) != T:
    raise ValueError("a future of %d steps downsampled by 0::%d has %d steps, not num_timesteps_to_keep=%d" %
                     (L, max(stride, 0), len(range(0, L, stride)) if stride >= 1 else 0, T))
  return stride


class DeviceCache:
  """A `pack_cache(..., targets=True)` cache resident in device memory, for training by the epoch
  (`DIMTrainer.train_epoch` / `CILTrainer.train_epoch`):

      data = DeviceCache(PackedCache(cache_dir), device)    # one upload: codes, lut, vec, future, mode
      batch = data.batch(rows, T, mode=False)                # the dict the trainers take, one kernel launch

  `batch(rows, T)` gathers rows `rows` (an int64 device tensor, or host indices that are range-checked) with
  `rip_gather_batch_u8`: `visual_features` [B,C,100,100] bit-identical to `transform_visual(lut[codes[rows]],
  channels_last=True)`, `velocity` [B,3], `is_at_traffic_light` [B,1], `traffic_light_state` [B,1] (views of one [B,5]
  tensor), `player_future` [B,T,2] = `future[rows, 0::L // T]` (the model's `transform`), and with `mode=True` the CIL
  `mode` [B,1] with STOP -> FORWARD (cil/model.py:166-168).  A device row outside [0, n) yields NaN for its row.

  The whole cache must fit in device memory (80 KB per 200 x 200 x 2 observation: 100 k observations are 8 GB); the
  constructor checks `torch.cuda.mem_get_info` first and raises MemoryError with the sizes otherwise.  Caches larger
  than device memory (a streamed variant) are not supported."""

  OUT_HW = 100

  def __init__(self, cache, device=None, staging_bytes: int = 64 << 20) -> None:
    if isinstance(cache, str):
      cache = PackedCache(cache)
    if not cache.has_targets:
      raise ValueError("DeviceCache: %s has no training targets; pack it with pack_cache(..., targets=True)" % cache.dir)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
      raise RuntimeError("DeviceCache needs a ROCm device, got %s (no CPU path)" % dev)
    if dev.index is None:
      dev = torch.device("cuda", torch.cuda.current_device())
    self.device = dev
    n, H, W, C = (int(v) for v in cache.codes.shape)
    L = int(cache.future.shape[1])
    self.n, self.H, self.W, self.C, self.L = n, H, W, C, L
    need = n * H * W * C + n * 4 * (5 + 2 * L + 1) + 256 * 4
    free, total = torch.cuda.mem_get_info(dev)
    if need > free:
      raise MemoryError("DeviceCache: the cache needs %.2f GB of device memory (%d observations: codes %.2f GB, targets "
                        "%.1f MB); %s has %.2f GB free of %.2f GB.  Caches larger than device memory are not supported." %
                        (need / 1e9, n, n * H * W * C / 1e9, n * 4 * (5 + 2 * L + 1) / 1e6, dev, free / 1e9, total / 1e9))
    with torch.cuda.device(dev):
      self.codes = torch.empty((n, H, W, C), dtype=torch.uint8, device=dev)
      per = max(1, int(staging_bytes) // (H * W * C))
      stream = torch.cuda.current_stream(dev)
      slots = [torch.empty((min(per, n), H, W, C), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
      done = [None, None]
      for k, i0 in enumerate(range(0, n, per)):  # memmap -> pinned slot -> device, the other slot's copy in flight
        m = min(per, n - i0)
        j = k & 1
        if done[j] is not None:
          done[j].synchronize()
        np.copyto(slots[j].numpy()[:m], cache.codes[i0:i0 + m])
        self.codes[i0:i0 + m].copy_(slots[j][:m], non_blocking=True)
        done[j] = torch.cuda.Event()
        done[j].record(stream)
      self.lut = torch.from_numpy(np.ascontiguousarray(cache.lut, np.float32)).to(dev)
      self.vec = torch.from_numpy(np.ascontiguousarray(cache.vec, np.float32)).to(dev)
      self.future = torch.from_numpy(np.array(cache.future, np.float32)).to(dev)
      self.mode = torch.from_numpy(np.array(cache.mode, np.float32)).to(dev)
      torch.cuda.synchronize(dev)  # the pinned slots are freed on return

  @classmethod
  def from_tensors(cls, codes, lut, vec, future, mode) -> "DeviceCache":
    """A `DeviceCache` around device tensors that already exist (`DeviceRecorder.cache`): codes [n,H,W,C] uint8,
    lut [256] float32, vec [n,5], future [n,L,2] and mode [n] float32, all contiguous and on one ROCm device.  Nothing is
    copied."""
    if not all(isinstance(t, torch.Tensor) for t in (codes, lut, vec, future, mode)):
      raise TypeError("DeviceCache.from_tensors takes torch tensors")
    if not codes.is_cuda:
      raise RuntimeError("DeviceCache needs a ROCm device, got %s (no CPU path)" % codes.device)
    for name, t, dt in (("codes", codes, torch.uint8), ("lut", lut, torch.float32), ("vec", vec, torch.float32),
                        ("future", future, torch.float32), ("mode", mode, torch.float32)):
      if t.dtype != dt:
        raise ValueError("DeviceCache.from_tensors: %s must be %s, got %s" % (name, dt, t.dtype))
      if t.device != codes.device:
        raise RuntimeError("DeviceCache.from_tensors: %s is on %s, codes on %s" % (name, t.device, codes.device))
      if not t.is_contiguous():
        raise ValueError("DeviceCache.from_tensors: %s is not contiguous" % name)
    if codes.dim() != 4:
      raise ValueError("DeviceCache.from_tensors: codes must have shape [n,H,W,C], got %s" % (tuple(codes.shape),))
    n, H, W, C = (int(v) for v in codes.shape)
    from oatomobile_amd import _lib
    _lib.expect_shape(lut, (256,), "lut")
    _lib.expect_shape(vec, (n, 5), "vec")
    _lib.expect_shape(future, (n, None, 2), "future")
    _lib.expect_shape(mode, (n,), "mode")
    if int(future.shape[1]) < 1:
      raise ValueError("DeviceCache.from_tensors: future has no steps")
    self = cls.__new__(cls)
    self.device = codes.device
    self.n, self.H, self.W, self.C, self.L = n, H, W, C, int(future.shape[1])
    self.codes, self.lut, self.vec, self.future, self.mode = codes, lut, vec, future, mode
    return self

  def __len__(self) -> int:
    return self.n

  @property
  def channels(self) -> int:
    return self.C

  def rows(self, rows) -> torch.Tensor:
    """`rows` as a contiguous int64 device tensor; host indices are range-checked here (device ones are not: that
    would synchronise — the kernel turns an out-of-range row into NaN outputs instead)."""
    if isinstance(rows, torch.Tensor) and rows.is_cuda:
      if rows.dtype.is_floating_point or rows.dim() != 1:
        raise ValueError("rows must be a 1-D integer tensor, got %s %s" % (rows.dtype, tuple(rows.shape)))
      return rows.to(self.device, torch.int64).contiguous()
    r = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows)
    if r.ndim != 1 or not np.issubdtype(r.dtype, np.integer):
      raise ValueError("rows must be 1-D integers, got %s %s" % (r.dtype, r.shape))
    if r.size and (r.min() < 0 or r.max() >= self.n):
      raise IndexError("rows outside [0, %d): min %d, max %d" % (self.n, r.min(), r.max()))
    return torch.from_numpy(r.astype(np.int64)).to(self.device)

  def batch(self, rows, T: int, mode: bool = False):
    """The trainer batch of `rows` with a target of `T` steps (ValueError if `future[:, 0::L // T]` has not T steps)."""
    from oatomobile_amd import _lib
    stride = downsample_stride(self.L, T)
    rows = self.rows(rows)
    B = int(rows.numel())
    if B == 0:
      raise ValueError("DeviceCache.batch: no rows")
    dev = self.device
    visual = torch.empty((B, self.C, self.OUT_HW, self.OUT_HW), device=dev)
    vec = torch.empty((B, 5), device=dev)
    target = torch.empty((B, T, 2), device=dev)
    mode_out = torch.empty((B, 1), device=dev) if mode else None
    with torch.cuda.device(dev):  # stateless entry point: launches on the current device
      _lib.check(_lib.load().rip_gather_batch_u8(
          _lib.ptr(self.codes, torch.uint8), _lib.ptr(self.lut), _lib.ptr(rows, torch.int64), B, self.n, self.C, self.H,
          self.W, self.OUT_HW, _lib.ptr(self.vec), _lib.ptr(self.future), self.L, int(T), stride, _lib.ptr(self.mode),
          _lib.ptr(visual), _lib.ptr(vec), _lib.ptr(target), _lib.ptr(mode_out), _lib.current_stream(dev)))
    out = dict(visual_features=visual, velocity=vec[:, 0:3], is_at_traffic_light=vec[:, 3:4],
               traffic_light_state=vec[:, 4:5], player_future=target)
    if mode:
      out["mode"] = mode_out
    return out


class DeviceRecorder:
  """Records driving on the device and labels it in hindsight: the way from what an agent just drove to a
  `DeviceCache` the trainers take, without a file and without a host copy of the observations.

      rec = DeviceRecorder.from_cache(train_cache, capacity=2000)     # the training set's table and BEV shape
      rec.append(lidar=..., velocity=..., is_at_traffic_light=..., traffic_light_state=..., location=..., rotation=...)
      rec.end_episode()                                               # windows do not cross this
      data = rec.cache()                                              # DeviceCache of the frames with a full window

  `append` takes host arrays or device tensors, codes the BEV against the fixed table with `rip_code_bev_u8` into row n
  of a preallocated [capacity,H,W,C] uint8 tensor, stores vec and the pose beside it and does not synchronise; more
  than `capacity` frames raise IndexError (from the host-side count).  `cache(num_frame_skips)` labels the frames
  `range(P, len - L, skips)` of every episode with one `rip_hindsight_targets` launch, compacts their rows and returns
  `DeviceCache.from_tensors(...)`; its one synchronisation reads the miss counter: a cell value that is not in the
  table is a ValueError with the count (such a recording needs a cache packed from its own data).  `frames` holds the
  labelled frame indices after `cache()`.  `lut` is a cache's `lut.npy` ([256] float32, NaN padded)."""

  def __init__(self, capacity: int, shape, lut, device=None, future_length: int = 80, past_length: int = 20,
               num_goals: int = 10, goal_stride: int = 8) -> None:
    dev = _cuda_device("cuda" if device is None else device, "DeviceRecorder")
    self.device, self.capacity = dev, int(capacity)
    self.H, self.W, self.C = (int(v) for v in shape)
    self.L, self.P, self.G, self.goal_stride = int(future_length), int(past_length), int(num_goals), int(goal_stride)
    if self.capacity < 1 or min(self.H, self.W, self.C) < 1 or self.L < 1 or self.P < 0:
      raise ValueError("DeviceRecorder: capacity, shape and future_length must be >= 1, past_length >= 0")
    lut = np.ascontiguousarray(lut.detach().cpu().numpy() if isinstance(lut, torch.Tensor) else lut, dtype=np.float32)
    if lut.shape != (256,):
      raise ValueError("DeviceRecorder: lut must have shape [256], got %s" % (lut.shape,))
    self.n_values = int((~np.isnan(lut)).sum())
    bits = lut.view(np.uint32)[:self.n_values].astype(np.int64)
    if self.n_values < 1 or np.isnan(lut[:self.n_values]).any() or (np.diff(bits) <= 0).any():
      raise ValueError("DeviceRecorder: lut is not a cache's table (ascending bit patterns, then NaN padding)")
    with torch.cuda.device(dev):
      self.lut = torch.from_numpy(lut).to(dev)
      self.codes = torch.empty((self.capacity, self.H, self.W, self.C), dtype=torch.uint8, device=dev)
      self.vec = torch.empty((self.capacity, 5), device=dev)
      self.location = torch.empty((self.capacity, 3), device=dev)
      self.rotation = torch.empty((self.capacity, 3), device=dev)
      self._miss = torch.zeros((1,), dtype=torch.int32, device=dev)  # a uint32 counter (rip_code_bev_u8)
    self._n, self._episode, self._episodes = 0, 0, []
    self.frames = None

  @classmethod
  def from_cache(cls, cache, capacity: int, device=None, **kwargs) -> "DeviceRecorder":
    """A recorder with the table and BEV shape of an existing `PackedCache` or `DeviceCache` (record with the training
    set's table); on the `DeviceCache`'s device unless `device` says otherwise."""
    if isinstance(cache, DeviceCache):
      return cls(capacity, (cache.H, cache.W, cache.C), cache.lut, cache.device if device is None else device, **kwargs)
    return cls(capacity, cache.codes.shape[1:], cache.lut, device, **kwargs)

  def __len__(self) -> int:
    return self._n

  def _f32(self, value, numel: int, what: str) -> torch.Tensor:
    if isinstance(value, torch.Tensor):
      t = value.to(self.device, torch.float32, non_blocking=True)
    else:
      t = torch.from_numpy(np.ascontiguousarray(np.asarray(value, dtype=np.float32))).to(self.device, non_blocking=True)
    if t.numel() != numel:
      raise ValueError("DeviceRecorder.append: %s has %d values, expected %d" % (what, t.numel(), numel))
    return t.reshape(-1)

  def append(self, *, lidar, velocity, is_at_traffic_light, traffic_light_state, location, rotation) -> None:
    from oatomobile_amd import _lib
    n = self._n
    if n >= self.capacity:
      raise IndexError("DeviceRecorder: frame %d exceeds the capacity of %d frames" % (n + 1, self.capacity))
    if tuple(np.shape(lidar)) != (self.H, self.W, self.C):
      raise ValueError("DeviceRecorder.append: lidar has shape %s, expected %s" % (tuple(np.shape(lidar)), (self.H, self.W, self.C)))
    bev = self._f32(lidar, self.H * self.W * self.C, "lidar").contiguous()
    self.vec[n, 0:3] = self._f32(velocity, 3, "velocity")
    self.vec[n, 3:4] = self._f32(is_at_traffic_light, 1, "is_at_traffic_light")
    self.vec[n, 4:5] = self._f32(traffic_light_state, 1, "traffic_light_state")
    self.location[n] = self._f32(location, 3, "location")
    self.rotation[n] = self._f32(rotation, 3, "rotation")
    with torch.cuda.device(self.device):  # stateless entry point: launches on the current device
      _lib.check(_lib.load().rip_code_bev_u8(_lib.ptr(bev), 1, self.H, self.W, self.C, _lib.ptr(self.lut), self.n_values,
                                             _lib.ptr(self.codes[n], torch.uint8), _lib.ptr(self._miss, torch.int32),
                                             _lib.current_stream(self.device)))
    self._episodes.append(self._episode)
    self._n = n + 1

  def end_episode(self) -> None:
    """Marks an episode boundary: no window reaches across it."""
    self._episode += 1

  def window_frames(self, num_frame_skips: int = 1) -> np.ndarray:
    """`range(P, len(episode) - L, num_frame_skips)` of every recorded episode, as indices into the recording."""
    episodes = np.asarray(self._episodes, np.int64)
    out = []
    for e in np.unique(episodes):
      idx = np.flatnonzero(episodes == e)  # contiguous: frames are appended in order
      out.append(idx[0] + np.arange(self.P, idx.size - self.L, int(num_frame_skips), dtype=np.int64))
    return np.concatenate(out).astype(np.int32) if out else np.empty((0,), np.int32)

  def cache(self, num_frame_skips: int = 1) -> "DeviceCache":
    if int(num_frame_skips) < 1:
      raise ValueError("DeviceRecorder.cache: num_frame_skips must be >= 1")
    frames = self.window_frames(num_frame_skips)
    if frames.size == 0:
      raise ValueError("DeviceRecorder.cache: no frame of the %d recorded has a full window (past %d, future %d)" %
                       (self._n, self.P, self.L))
    dev, n = self.device, self._n
    with torch.cuda.device(dev):
      rows = torch.from_numpy(frames).to(dev)
      episode = torch.from_numpy(np.asarray(self._episodes, np.int32)).to(dev)
      out = _hindsight_launch(self.location[:n], self.rotation[:n], episode, rows, self.L, self.P, self.G, self.goal_stride,
                              {"future_xy", "mode"})
      index = rows.to(torch.int64)
      codes, vec = self.codes.index_select(0, index), self.vec.index_select(0, index)
      misses = int(self._miss.item()) & 0xffffffff  # the one synchronisation
    if misses:
      raise ValueError("DeviceRecorder.cache: %d recorded BEV cells hold a value that is not in the table" % misses)
    self.frames = frames
    return DeviceCache.from_tensors(codes, self.lut, vec, out["future_xy"], out["mode"])


def replay_cache(agent, cache: "PackedCache", batch_size: int, interpolate: bool = False, begin: int = 0,
                 end: Optional[int] = None, streams: int = 1, stats: bool = False):
  """`replay()` from a packed cache: plans of observations [begin, end) -> [n,4,2] float32, or with `interpolate` the
  [n,30,3] float64 plans `agent(observation)` returns.  Per batch: one memcpy out of the page cache into pinned staging
  (80 KB per observation), H2D on a copy stream under the previous batch's kernels, `RIPAgent.plan_batch_coded`, D2H of
  the plans into pinned memory.  Ranks of a multi-GPU job take `distributed.shard_range(len(cache), rank, world)`.
  `streams=2` (round 6): even batches run on `agent`, odd batches on `agent.twin()` — a second handle — each on a stream
  of its own, so that one batch's encoder launches (whose grids leave CUs idle at their tails) run beside the other
  batch's search; the plans are the same bits (same kernels, same inputs, rows written to disjoint slices of the result).
  `stats=True` returns `(plans, stats [n,4] float32, q [n,K] float32)`: per observation the ensemble disagreement of its
  plan (`RIPAgent.plan_batch_coded(return_stats=True)`: mean, population variance, min, max of the K members' log q_k,
  and the K values), rows in the same disjoint slices."""
  if streams not in (1, 2):
    raise ValueError("replay_cache: streams must be 1 or 2")
  dev = agent._device
  end = len(cache) if end is None else end
  n = max(0, end - begin)
  shape, ndt, tdt = ((n, 30, 3), np.float64, torch.float64) if interpolate else ((n, 4, 2), np.float32, torch.float32)
  out = torch.empty(shape, dtype=tdt, pin_memory=True)
  K = len(agent._models)
  out_s = torch.empty((n, 4), dtype=torch.float32, pin_memory=True) if stats else None
  out_q = torch.empty((n, K), dtype=torch.float32, pin_memory=True) if stats else None
  if n == 0:
    return (out.numpy(), out_s.numpy(), out_q.numpy()) if stats else out.numpy()
  lut = torch.from_numpy(cache.lut).to(dev)
  copy = torch.cuda.Stream(device=dev)
  main = torch.cuda.current_stream(dev)
  if streams == 2:
    agents = [agent, agent.replay_twin()]  # (weights and handle options follow the agent's: RIPAgent.replay_twin)
    lanes = [torch.cuda.Stream(device=dev) for _ in range(2)]
    for s in lanes:
      s.wait_stream(main)
  else:
    agents, lanes = [agent, agent], [main, main]
  H, W, C = cache.codes.shape[1:]
  G = cache.goal.shape[1]
  dslots = [(torch.empty((batch_size, H, W, C), dtype=torch.uint8, device=dev), torch.empty((batch_size, 5), device=dev),
             torch.empty((batch_size, G, 2), device=dev)) for _ in range(2)]
  ready = [torch.cuda.Event() for _ in range(2)]
  freed = [torch.cuda.Event() for _ in range(2)]
  filled = [torch.cuda.Event() for _ in range(2)]  # the host slot's H2D is done: `batches()` may overwrite it
  for j in range(2):
    freed[j].record(lanes[j])
  i0 = 0
  it = cache.batches(batch_size, begin, end)
  for k in range((n + batch_size - 1) // batch_size):
    j = k & 1
    if k >= 2:
      filled[j].synchronize()  # the generator refills host slot j now: its previous upload must have left it
    c, v, g = next(it)
    m = c.shape[0]
    with torch.cuda.stream(copy):
      copy.wait_event(freed[j])
      dslots[j][0][:m].copy_(c, non_blocking=True)
      dslots[j][1][:m].copy_(v, non_blocking=True)
      dslots[j][2][:m].copy_(g, non_blocking=True)
      ready[j].record(copy)
      filled[j].record(copy)
    with torch.cuda.stream(lanes[j]):  # (one stream: the current stream itself)
      lanes[j].wait_event(ready[j])
      if stats:
        plan, ps = agents[j].plan_batch_coded(dslots[j][0][:m], lut, dslots[j][1][:m], dslots[j][2][:m],
                                              interpolate=interpolate, return_stats=True)
        out_s[i0:i0 + m].copy_(torch.stack((ps.mean, ps.variance, ps.min, ps.max), dim=1), non_blocking=True)
        out_q[i0:i0 + m].copy_(ps.q.t(), non_blocking=True)
      else:
        plan = agents[j].plan_batch_coded(dslots[j][0][:m], lut, dslots[j][1][:m], dslots[j][2][:m], interpolate=interpolate)
      out[i0:i0 + m].copy_(plan, non_blocking=True)
      freed[j].record(lanes[j])
    i0 += m
  torch.cuda.synchronize(dev)
  return (out.numpy(), out_s.numpy(), out_q.numpy()) if stats else out.numpy()


def score_cache(agent, data: "DeviceCache", batch_size: int) -> dict:
  """The per-member expert log-likelihood and its ensemble statistics over a whole device-resident cache, one pass:
  for every row the trajectory is the expert's future as the model sees it (`data.batch(rows, 4)["player_future"]` =
  `future[:, 0::L // 4]`), the batch's already transformed `visual_features` go through `rip_encode` for the K members
  of `agent` (a `RIPAgent` with `max_batch >= batch_size`), then one `rip_plan_stats` launch per batch.
  -> dict(q [n,K] float32 = log q_k(expert | x), stats [n,4] float32 = its mean, population variance, min, max over k)."""
  from oatomobile_amd import _lib, arch
  dev = agent._device
  if data.device != dev:
    raise RuntimeError("score_cache: the cache is on %s, the agent on %s" % (data.device, dev))
  if data.channels != agent._in_channels:
    raise ValueError("score_cache: the cache has %d BEV channels, the agent expects %d" % (data.channels, agent._in_channels))
  batch_size = int(batch_size)
  if batch_size < 1 or batch_size > agent._max_batch:
    raise ValueError("score_cache: batch_size %d outside [1, max_batch=%d]" % (batch_size, agent._max_batch))
  n, K = len(data), len(agent._models)
  if agent._sync_weights():
    agent._online = {}
  q = torch.empty((n, K), device=dev, dtype=torch.float32)
  stats = torch.empty((n, _lib.STAT_SLOTS), device=dev, dtype=torch.float32)
  lib, h = _lib.load(), agent._handle
  z = torch.empty((K, batch_size, 64), device=dev, dtype=torch.float32)
  qb = torch.empty((K, batch_size), device=dev, dtype=torch.float32)
  agent._eager_pending = True
  for i0 in range(0, n, batch_size):
    m = min(batch_size, n - i0)
    batch = data.batch(torch.arange(i0, i0 + m, device=dev), arch.T)
    vec = torch.cat((batch["velocity"], batch["is_at_traffic_light"], batch["traffic_light_state"]), dim=1)  # [m,5]
    zb, qv = z.view(-1)[:K * m * 64].view(K, m, 64), qb.view(-1)[:K * m].view(K, m)
    st = h.stream()
    _lib.check(lib.rip_encode(h.raw, _lib.ptr(batch["visual_features"]), _lib.ptr(vec), m, 0, K, agent._enc_dtype,
                              _lib.ptr(zb), None, st))
    _lib.check(lib.rip_plan_stats(h.raw, _lib.ptr(zb), _lib.ptr(batch["player_future"]), m, 1, _lib.ptr(qv),
                                  _lib.ptr(stats[i0:i0 + m]), st))
    q[i0:i0 + m].copy_(qv.t())
  torch.cuda.synchronize(dev)
  return dict(q=q.cpu().numpy(), stats=stats.cpu().numpy())


def predict_cache(agent, data: "DeviceCache", batch_size: int, num_samples: int, top_k: int, seed: int = 0) -> dict:
  """Open-loop evaluation of the ensemble over a whole device-resident cache, one pass: per batch of rows [i0, i0 + m)
  `data.batch(rows, 4)` gives the transformed visual features, vec and the expert's future as the target, `rip_encode`
  the z of the K members of `agent` (a `RIPAgent` with `max_batch >= batch_size`), and `rip_predict` with `row0 = i0`
  draws `num_samples` trajectories per member, ranks all K x num_samples of them by the agent's algorithm (no goal) and
  measures the best `top_k` against the expert.  Sample ids are counted from the row's index in the cache, so the
  result does not depend on `batch_size` (a rank that takes `distributed.shard_range` of the rows passes nothing else).
  -> dict(ade, fde, loss [n,k] float32, member [n,k] int32 best-first per row, and the data-set means
  min_ade_1, min_ade_k, min_fde_1, min_fde_k: floats)."""
  from oatomobile_amd import _lib, arch, prediction
  dev = agent._device
  if data.device != dev:
    raise RuntimeError("predict_cache: the cache is on %s, the agent on %s" % (data.device, dev))
  if data.channels != agent._in_channels:
    raise ValueError("predict_cache: the cache has %d BEV channels, the agent expects %d" % (data.channels, agent._in_channels))
  batch_size = int(batch_size)
  if batch_size < 1 or batch_size > agent._max_batch:
    raise ValueError("predict_cache: batch_size %d outside [1, max_batch=%d]" % (batch_size, agent._max_batch))
  n, K = len(data), len(agent._models)
  S, top_k = agent._check_predict("predict_cache", batch_size, num_samples, top_k, None, None, None, 0, seed)
  if agent._sync_weights():
    agent._online = {}
  h = agent._handle
  f32 = dict(device=dev, dtype=torch.float32)
  ade, fde, loss = (torch.empty((n, top_k), **f32) for _ in range(3))
  member = torch.empty((n, top_k), device=dev, dtype=torch.int32)
  z = torch.empty((K, batch_size, 64), **f32)
  agent._eager_pending = True
  for i0 in range(0, n, batch_size):
    m = min(batch_size, n - i0)
    batch = data.batch(torch.arange(i0, i0 + m, device=dev), arch.T)
    vec = torch.cat((batch["velocity"], batch["is_at_traffic_light"], batch["traffic_light_state"]), dim=1)  # [m,5]
    zb = z.view(-1)[:K * m * 64].view(K, m, 64)
    _lib.check(_lib.load().rip_encode(h.raw, _lib.ptr(batch["visual_features"]), _lib.ptr(vec), m, 0, K, agent._enc_dtype,
                                      _lib.ptr(zb), None, h.stream()))
    p = agent._predict(zb, m, S, top_k, None, batch["player_future"], None, seed, i0, False)
    ade[i0:i0 + m], fde[i0:i0 + m], loss[i0:i0 + m], member[i0:i0 + m] = p.ade, p.fde, p.loss, p.member
  torch.cuda.synchronize(dev)
  out = dict(ade=ade.cpu().numpy(), fde=fde.cpu().numpy(), loss=loss.cpu().numpy(), member=member.cpu().numpy())
  for name in ("ade", "fde"):
    for tag, k in (("1", 1), ("k", top_k)):  # means in float64 of the float32 rows
      out["min_%s_%s" % (name, tag)] = float(prediction.min_over_k(out[name], k).astype(np.float64).mean()) if n else float("nan")
  return out


class FeatureCache:
  """The K members' encoder outputs over a whole `DeviceCache`, what `train.HeadTrainer` trains on:

      cache = FeatureCache.build(agent, data, batch_size=128)   # feat [K,n,128] on the device, 2 KB per observation at K = 4
      cache.verify(agent)                                        # a few rows recomputed and compared bit for bit

  `feat[k, i]` is member k's MobileNetV2 logits on observation i (`RIPAgent.features_batch_coded` on the cache's rows
  [i0, i0 + batch_size) in order); `vec` [n,5] and `future` [n,L,2] are the `DeviceCache`'s own tensors (shared, not
  copied).  The cache is valid only while the members' ENCODERS are unchanged: a head update (`HeadTrainer.publish`)
  leaves it valid, anything that loads other encoder weights into the agent does not, and nothing invalidates it
  automatically — `verify` is the check.  The encoder's kernel selection keys on B * K, so the features are
  reproducible bit for bit only at the same batch composition: `verify` recomputes the batches of `batch_size` rows
  the cache was built with."""

  def __init__(self, feat: torch.Tensor, vec: torch.Tensor, future: torch.Tensor, batch_size: int, data: "DeviceCache") -> None:
    self.feat, self.vec, self.future, self.batch_size, self.data = feat, vec, future, int(batch_size), data

  def __len__(self) -> int:
    return int(self.feat.shape[1])

  @staticmethod
  def _batch(agent, data: "DeviceCache", i0: int, i1: int) -> torch.Tensor:
    feat, _ = agent.features_batch_coded(data.codes[i0:i1], data.lut, data.vec[i0:i1])
    return feat

  @classmethod
  def build(cls, agent, data: "DeviceCache", batch_size: int) -> "FeatureCache":
    dev = agent._device
    if data.device != dev:
      raise RuntimeError("FeatureCache.build: the cache is on %s, the agent on %s" % (data.device, dev))
    if data.channels != agent._in_channels:
      raise ValueError("FeatureCache.build: the cache has %d BEV channels, the agent expects %d" % (data.channels, agent._in_channels))
    batch_size = int(batch_size)
    if batch_size < 1 or batch_size > agent._max_batch:
      raise ValueError("FeatureCache.build: batch_size %d outside [1, max_batch=%d]" % (batch_size, agent._max_batch))
    n, K = len(data), len(agent._models)
    feat = torch.empty((K, n, 128), device=dev, dtype=torch.float32)
    for i0 in range(0, n, batch_size):
      i1 = min(n, i0 + batch_size)
      feat[:, i0:i1] = cls._batch(agent, data, i0, i1)
    return cls(feat, data.vec, data.future, batch_size, data)

  def verify(self, agent, rows: int = 8) -> bool:
    """Recomputes the build batches of `rows` rows spread evenly over the cache with `agent` and compares them with the
    cached features bit for bit (one synchronisation).  False = the members' encoders are not the ones the cache was
    built with (or the agent's batch composition differs): rebuild."""
    n = len(self)
    picks = sorted({(j * n) // max(1, int(rows)) for j in range(max(1, int(rows)))})
    same = torch.ones((), dtype=torch.bool, device=self.feat.device)
    for b0 in sorted({(i // self.batch_size) * self.batch_size for i in picks}):
      b1 = min(n, b0 + self.batch_size)
      fresh = self._batch(agent, self.data, b0, b1)
      same = same & (fresh.view(torch.int32) == self.feat[:, b0:b1].view(torch.int32)).all()
    return bool(same)
