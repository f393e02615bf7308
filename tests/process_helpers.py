"""Shared by tests/test_process_cpu.py and tests/test_record.py: the raw episodes of tests/golden/g17_process.npz
(written by the reference's `Episode.append`, labelled by the reference's `CARLADataset.process`:
tools/make_golden_process.py) rebuilt with `replay.Episode`."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_process.npz")
RAW_KEYS = ("location", "rotation", "lidar", "velocity", "is_at_traffic_light", "traffic_light_state")
F64_TOL = 1e-10  # metres: player_future / player_past against the reference (derived in the issue: ~10 float64 operations
                 # on differences of a few hundred metres deviate by ~1e-12 m, two orders of margin)


def g17():
  with np.load(GOLDEN) as g:
    return {k: g[k] for k in g.files}


def case_params(g, case):
  L, P, skips = (int(v) for v in g["%s_params" % case])
  return L, P, skips


def episode_raw(g, case, ep):
  """-> (tokens, {key: [n, ...] array}) of one raw episode."""
  return [str(t) for t in g["%s_%s_tokens" % (case, ep)]], {k: g["%s_%s_%s" % (case, ep, k)] for k in RAW_KEYS}


def write_raw(g, case, parent_dir):
  """The raw dataset of `case` under `parent_dir`, one `replay.Episode` per episode with the fixture's sample tokens."""
  from oatomobile_amd import replay
  for ep in g["%s_episodes" % case]:
    tokens, raw = episode_raw(g, case, str(ep))
    episode = replay.Episode(str(parent_dir), str(ep))
    for i, token in enumerate(tokens):
      episode.append(token, **{k: raw[k][i] for k in RAW_KEYS})
  return str(parent_dir)


def ulp_distance(a, b):
  """Largest distance in float32 units in the last place between two finite float32 arrays of one shape."""
  a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
  assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
  ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
  ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
  return int(np.abs(ia - ib).max()) if a.size else 0
