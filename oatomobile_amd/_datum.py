"""Datum decode and cache packing without torch (numpy only).

Imported by `replay.py`, and run as a SCRIPT by `replay.pack_cache`'s worker processes (`python _datum.py <job.json>`):
a packing worker must not pay `import torch` + the HIP library (2 s each) for 0.1 s of numpy work, and must not inherit
the parent's HIP context through a fork — so this file has no package-relative imports.

Reference formats: datum files `oatomobile/datasets/carla.py:107-164`; the goal derivation is SURVEY.md 8(d) config 5.
"""

import io
import json
import os
import sys
from typing import Mapping, Sequence

import numpy as np

MODALITIES = ("lidar", "velocity", "is_at_traffic_light", "traffic_light_state", "player_future")


def load_datum(fname: str, modalities: Sequence[str] = MODALITIES, mode: bool = False,
               dataformat: str = "HWC") -> Mapping[str, np.ndarray]:
  """datasets/carla.py:107-164: float32 casts, scalars -> 1-D, optional HWC->CHW, optional driving-mode label
  ({0 FORWARD, 1 STOP, 2 LEFT, 3 RIGHT} from the last future waypoint), `name` = path."""
  assert dataformat in ("HWC", "CHW")
  sample = {}
  with open(fname, "rb") as f:  # one read of the (small, compressed) file: the zip directory walk then costs no syscalls
    blob = io.BytesIO(f.read())
  with np.load(blob) as datum:
    for attr in modalities:
      v = np.atleast_1d(datum[attr]).astype(np.float32)
      if v.ndim == 3 and dataformat == "CHW":
        v = np.transpose(v, (2, 0, 1))
      sample[attr] = v
  if mode and "player_future" in sample:
    sample["mode"] = np.atleast_1d(mode_label(sample["player_future"])).astype(np.float32)
  sample["name"] = fname
  return sample


def mode_label(player_future: np.ndarray) -> int:
  """datasets/carla.py:148-162: the driving-mode label of a datum from its last future waypoint."""
  x_T, y_T = player_future[-1, :2]
  norm = np.linalg.norm([x_T, y_T])
  theta = np.degrees(np.arccos(x_T / (norm + 1e-3)))
  return 1 if norm < 3 else (2 if theta > 15 else (3 if theta <= -15 else 0))


def goal_from_future(player_future: np.ndarray, num_goals: int = 10, stride: int = 8) -> np.ndarray:
  """`player_future[stride-1::stride][:num_goals, :2]`, padded by repeating the last waypoint."""
  g = np.asarray(player_future, dtype=np.float32)[stride - 1::stride][:num_goals, :2]
  if g.shape[0] < num_goals:
    g = np.concatenate([g, np.repeat(g[-1:], num_goals - g.shape[0], axis=0)], axis=0)
  return g


def rot2mat(rotation: np.ndarray) -> np.ndarray:
  """utils/carla.py:642-649, as `agents.rot2mat` writes it out (this file imports nothing of the package):
  `euler2mat(roll, pitch, yaw).T` (static 'sxyz') of (pitch, yaw, roll) in degrees, float64."""
  pitch, yaw, roll = np.deg2rad(np.asarray(rotation, dtype=np.float64))
  ci, si = np.cos(roll), np.sin(roll)
  cj, sj = np.cos(pitch), np.sin(pitch)
  ck, sk = np.cos(yaw), np.sin(yaw)
  cc, cs, sc, ss = ci * ck, ci * sk, si * ck, si * sk
  m = np.array([[cj * ck, sj * sc - cs, sj * cc + ss], [cj * sk, sj * ss + cc, sj * cs - sc], [-sj, cj * si, cj * ci]])
  return m.T


def hindsight_targets(location: np.ndarray, rotation: np.ndarray, frames: Sequence[int], L: int, P: int, episode=None):
  """`CARLADataset.process`'s labels (datasets/carla.py:278-313) for the windows `frames` of a pose track, the numpy
  restatement of `rip_hindsight_targets`: -> (player_future [M,L,3], player_past [M,P,3]) float64, window m being frame
  i = frames[m], `world2local` (utils/carla.py:651-674) of frames i+1..i+L and i-P..i-1 about frame i.  The same
  operations in the same precisions as the reference on recorded data: `world_locations - current_location` in the
  dtype of `location` (float32 from the sensors), the matrix and the product in float64.  A window that leaves [0, N)
  or — with `episode` [N], the episode number of every frame — crosses an episode boundary is all NaN."""
  location, rotation = np.asarray(location), np.asarray(rotation)
  N, L, P = location.shape[0], int(L), int(P)
  frames = np.asarray(frames, dtype=np.int64).reshape(-1)
  future = np.full((frames.size, L, 3), np.nan, np.float64)
  past = np.full((frames.size, P, 3), np.nan, np.float64)
  for m, i in enumerate(frames):
    i = int(i)
    if i - P < 0 or i + L >= N or (episode is not None and not episode[i - P] == episode[i] == episode[i + L]):
      continue
    R = rot2mat(rotation[i])
    future[m] = np.dot(R, (location[i + 1:i + 1 + L] - location[i]).T).T
    if P:
      past[m] = np.dot(R, (location[i - P:i] - location[i]).T).T
  return future, past


def targets_from_future(player_future: np.ndarray, num_goals: int, goal_stride: int):
  """What `_fill_rows` derives from the `player_future` [n,L,3] of n datums, as `load_datum` hands it over (float32):
  -> future [n,L,2], goal [n,G,2], mode [n], all float32."""
  pf = np.asarray(player_future).astype(np.float32)
  goal = np.empty((pf.shape[0], num_goals, 2), np.float32)
  mode = np.empty((pf.shape[0],), np.float32)
  for j in range(pf.shape[0]):
    goal[j] = goal_from_future(pf[j], num_goals, goal_stride)
    mode[j] = mode_label(pf[j])
  return np.ascontiguousarray(pf[:, :, :2]), goal, mode


def _fill_rows(files, j0, lidar, vec, goal, num_goals, goal_stride, future=None, mode=None, labelled=True):
  """Decodes `files` into rows j0.. of the batch arrays (numpy views; shared memory in the worker processes); with
  `future` / `mode` also the training targets `player_future[:, :2]` and `load_datum(mode=True)`'s label.
  `labelled=False`: raw samples, which have no `player_future` — only `lidar` and `vec` are filled."""
  for j, f in enumerate(files, start=j0):
    d = load_datum(f) if labelled else load_datum(f, modalities=MODALITIES[:-1])
    lidar[j] = d["lidar"]
    vec[j, :3] = d["velocity"].reshape(3)
    vec[j, 3] = float(d["is_at_traffic_light"].reshape(-1)[0])
    vec[j, 4] = float(d["traffic_light_state"].reshape(-1)[0])
    if not labelled:
      continue
    goal[j] = goal_from_future(d["player_future"], num_goals, goal_stride)
    if future is not None:
      future[j] = d["player_future"][:, :2]
      mode[j] = mode_label(d["player_future"])
  return len(files)



def code_bev(bits: np.ndarray, table: np.ndarray):
  """uint8 codes of a BEV given as uint32 BIT PATTERNS against `table` (sorted distinct uint32 patterns), growing the
  table by the patterns it lacks.  Returns (codes, table).  Working on bit patterns keeps -0.0 and +0.0 apart (float
  comparison merges them) — `table.view(float32)[codes]` is the input bit for bit.  NaN patterns raise."""
  flat = bits.reshape(-1)
  if table.size:
    c = np.minimum(np.searchsorted(table, flat), table.size - 1)
    miss = table[c] != flat
    if miss.any():
      table = np.union1d(table, np.unique(flat[miss])).astype(np.uint32)
      c = np.searchsorted(table, flat)
      if not np.array_equal(table[c], flat):
        raise RuntimeError("pack_cache: table lookup does not reproduce the BEV")  # cannot happen
  else:
    table = np.unique(flat).astype(np.uint32)
    c = np.searchsorted(table, flat)
  if np.isnan(table.view(np.float32)).any():
    raise ValueError("pack_cache: NaN in a BEV")
  if table.size > 256:
    raise ValueError("pack_cache: more than 256 distinct BEV values (%d): not a clipped histogram" % table.size)
  return c.astype(np.uint8).reshape(bits.shape), table


def pack_span(files, i0, out_dir, shape, num_goals, goal_stride, chunk, future_len=0, labels=None):
  """Packs `files` into rows i0.. of `<out_dir>/codes.npy` (an existing memmap of `shape`), one datum at a time through
  a reused frame buffer (a chunk-sized float32 staging array costs more in first-touch page faults than the decode),
  coded against the table of THIS span as known so far; when a datum brings a new value the rows of the current chunk
  are re-coded at once, so every chunk is consistent with one table.  Returns [(row0, rows, that table)], vec, goal,
  future, mode: the parent unifies the tables and re-codes the chunks whose table differs from the final one.
  `future_len` > 0: also the training targets, future [m, future_len, 2] and mode [m] (else both None).
  `labels` = (future, goal, mode) of these rows, already derived: `files` are then raw samples without a
  `player_future` (`replay.pack_episodes`), and these arrays are returned as they are."""
  n, H, W, C = shape
  codes = np.lib.format.open_memmap(os.path.join(out_dir, "codes.npy"), mode="r+")
  assert codes.shape == tuple(shape) and codes.dtype == np.uint8
  vec = np.empty((len(files), 5), np.float32)
  goal = np.empty((len(files), num_goals, 2), np.float32)
  future = np.empty((len(files), future_len, 2), np.float32) if future_len else None
  mode = np.empty((len(files),), np.float32) if future_len else None
  if labels is not None:
    future, goal, mode = labels
  table = np.empty((0,), np.uint32)
  frame = np.empty((1, H, W, C), np.float32)
  bits = frame.view(np.uint32)
  spans = []
  for j0 in range(0, len(files), chunk):
    part = files[j0:j0 + chunk]
    for j, f in enumerate(part, start=j0):
      _fill_rows([f], 0, frame, vec[j:j + 1], goal[j:j + 1], num_goals, goal_stride,
                 None if future is None else future[j:j + 1], None if mode is None else mode[j:j + 1], labels is None)
      c, grown = code_bev(bits, table)
      if grown.size != table.size and j > j0:  # a new value inside the chunk: its earlier rows move to the new table
        remap = np.searchsorted(grown, table).astype(np.uint8)
        codes[i0 + j0:i0 + j] = remap[codes[i0 + j0:i0 + j]]
      table = grown
      codes[i0 + j] = c[0]  # code_bev compared table[c] with the frame's bit patterns element by element
    spans.append((i0 + j0, len(part), table.copy()))
  codes.flush()
  del codes
  return spans, vec, goal, future, mode


if __name__ == "__main__":  # worker process of replay.pack_cache: `python _datum.py job.json` -> job["result"] (.npz)
  with open(sys.argv[1]) as fh:
    job = json.load(fh)
  try:
    spans, vec, goal, future, mode = pack_span(job["files"], job["i0"], job["out_dir"], tuple(job["shape"]),
                                               job["num_goals"], job["goal_stride"], job["chunk"], job.get("future_len", 0))
    targets = {} if future is None else dict(future=future, mode=mode)
    np.savez(job["result"], vec=vec, goal=goal, rows=np.array([(a, b) for a, b, _ in spans], np.int64),
             sizes=np.array([t.size for _, _, t in spans], np.int64),
             tables=np.concatenate([t for _, _, t in spans]) if spans else np.empty((0,), np.uint32), **targets)
  except ValueError as exc:  # refused data (NaN, > 256 values): the parent re-raises it as ValueError
    with open(job["result"] + ".err", "w") as fh:
      fh.write(str(exc))
    sys.exit(3)
