"""Sample-and-rank ensemble prediction: the host side of `rip_predict` (include/rip_hip.h).

`RIPAgent.predict_batch` draws S trajectories from every member's flow, scores all M = K S of them under all K members,
aggregates with the agent's WCM / MA / BCM and returns the best `top_k` as a `Prediction`; `replay.predict_cache` runs it
over a packed cache against the expert's future.  This module holds what needs no device: the numpy restatement of the
device generator (`philox_normal`), the displacement metrics and the result type.
"""

from typing import Any, NamedTuple

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57  # Philox4x32 multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85  # Weyl constants of the key schedule
MAX_CANDIDATES = 4096  # M = K S of one rip_predict call
MAX_TOP_K = 64


class Prediction(NamedTuple):
  """The `top_k` best candidates per observation in ascending order of loss: `y` [B,k,4,2], `loss` [B,k], `index` [B,k]
  (candidate m = j S + s of the [B,M] candidate set), `member` [B,k] (= index // S: whose flow drew it), and against a
  target `ade` / `fde` [B,k] (average / final displacement error in the units of y), else None."""
  y: Any
  loss: Any
  index: Any
  member: Any
  ade: Any
  fde: Any


def philox4x32(counter, key, rounds: int = 10) -> np.ndarray:
  """Philox4x32 (Salmon et al. 2011): counter [...,4], key [...,2] uint32 -> [...,4] uint32 words."""
  c = [np.asarray(counter, dtype=np.uint32)[..., i].astype(np.uint64) for i in range(4)]
  k = [np.asarray(key, dtype=np.uint32)[..., i].astype(np.uint64) for i in range(2)]
  mask = np.uint64(0xFFFFFFFF)
  s32 = np.uint64(32)
  for _ in range(rounds):
    p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]
    c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & mask, (p0 >> s32) ^ c[3] ^ k[1], p0 & mask]
    k = [(k[0] + np.uint64(PHILOX_W0)) & mask, (k[1] + np.uint64(PHILOX_W1)) & mask]
  return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def _box_muller(wa: np.ndarray, wb: np.ndarray):
  """One word pair -> two normals, every operation in float32."""
  scale = np.float32(2.0**-24)
  u = ((wa >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * scale  # (0, 1]
  v = (wb >> np.uint32(8)).astype(np.float32) * scale                   # [0, 1)
  r = np.sqrt(np.float32(-2.0) * np.log(u))
  a = np.float32(2.0 * np.pi) * v
  return r * np.cos(a), r * np.sin(a)


def philox_normal(seed: int, first_id: int, n: int) -> np.ndarray:
  """The device generator on the host: [n,8] float32, row i = the latent x[4][2] (flattened) of sample id
  `first_id + i` under `seed` — what `rip_sample_normal` writes and what `rip_predict` feeds member j's flow for
  sample id ((row0 + b) K + j) S + s.  Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
  (g & 0xffffffff, g >> 32, c, 0); call c in {0, 1} fills x[4c .. 4c+3] by Box-Muller on (w0, w1) and (w2, w3) in
  float32: u = ((wa >> 8) + 1) 2^-24, v = (wb >> 8) 2^-24 -> sqrt(-2 ln u) (cos, sin)(2 pi v)."""
  seed, first_id, n = int(seed), int(first_id), int(n)
  if n < 0 or not 0 <= seed < 2**64 or not 0 <= first_id < 2**64:
    raise ValueError("philox_normal: seed and first_id are unsigned 64-bit integers, n >= 0")
  g = (np.uint64(first_id) + np.arange(n, dtype=np.uint64))  # wraps modulo 2^64 like the device's counter
  key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
  out = np.empty((n, 8), dtype=np.float32)
  for c in (0, 1):
    counter = np.stack([(g & np.uint64(0xFFFFFFFF)).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32),
                        np.full(n, c, np.uint32), np.zeros(n, np.uint32)], axis=-1)
    w = philox4x32(counter, key)
    out[:, 4 * c + 0], out[:, 4 * c + 1] = _box_muller(w[:, 0], w[:, 1])
    out[:, 4 * c + 2], out[:, 4 * c + 3] = _box_muller(w[:, 2], w[:, 3])
  return out


def displacement_errors(y, target):
  """y [...,k,T,2] candidate trajectories, target [...,T,2] -> (ade, fde) [...,k] float64: the mean over the T steps of
  the Euclidean distance to the target, and the distance at the last step."""
  y, target = np.asarray(y, dtype=np.float64), np.asarray(target, dtype=np.float64)
  if y.ndim < 3 or y.shape[-1] != 2 or target.shape != y.shape[:-3] + y.shape[-2:]:
    raise ValueError("displacement_errors: y [...,k,T,2] and target [...,T,2], got %s and %s" % (y.shape, target.shape))
  d = np.sqrt(((y - target[..., None, :, :])**2).sum(-1))  # [...,k,T]
  return d.mean(-1), d[..., -1]


def min_over_k(err, k: int) -> np.ndarray:
  """minADE_k / minFDE_k per row: err [...,K'] ranked best-first (as `Prediction.ade`) -> the minimum over its first k."""
  err = np.asarray(err)
  if err.ndim < 1 or not 1 <= int(k) <= err.shape[-1]:
    raise ValueError("min_over_k: k=%s outside [1, %s]" % (k, err.shape[-1] if err.ndim else 0))
  return err[..., :int(k)].min(-1)
