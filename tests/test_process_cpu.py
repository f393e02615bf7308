"""CPU tests of hindsight labelling: `replay.process` against what the reference's `CARLADataset.process` wrote
(tests/golden/g17_process.npz), `replay.pack_episodes` against `pack_cache` of those datums, the numpy restatement
`_datum.hindsight_targets`, the two new entry points' bindings and the `--raw_dataset` flag.  No GPU needed."""
import os
import re

import numpy as np
import pytest

from tests import process_helpers as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CACHE_FILES = ("codes.npy", "lut.npy", "vec.npy", "goal.npy", "future.npy", "mode.npy")


@pytest.fixture(scope="module")
def g():
  return PH.g17()


@pytest.mark.parametrize("case", ["default", "short"])
def test_process_matches_the_reference(g, tmp_path, case):
  """Same file names; every raw key bit for bit (value and dtype); player_future / player_past within 1e-10 m."""
  from oatomobile_amd import replay
  L, P, skips = PH.case_params(g, case)
  raw = PH.write_raw(g, case, tmp_path / "raw")
  written = replay.process(raw, str(tmp_path / "out"), future_length=L, past_length=P, num_frame_skips=skips)
  want = [str(t) for t in g["%s_datums" % case]]
  assert sorted(os.listdir(tmp_path / "out")) == sorted(t + ".npz" for t in want)
  assert sorted(os.path.basename(f)[:-4] for f in written) == sorted(want)
  for token in want:
    prefix = "%s_datum_%s_" % (case, token)
    ref = {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}
    with np.load(tmp_path / "out" / (token + ".npz"), allow_pickle=True) as datum:
      assert sorted(datum.files) == sorted(ref)
      for k in PH.RAW_KEYS:
        assert datum[k].dtype == ref[k].dtype and datum[k].shape == ref[k].shape, k
        assert datum[k].tobytes() == ref[k].tobytes(), k  # bytes: the -0.0 of the lidar stays -0.0
      for k, rows in (("player_future", L), ("player_past", P)):
        assert datum[k].dtype == np.float64 and datum[k].shape == (rows, 3) == ref[k].shape
        err = float(np.abs(datum[k] - ref[k]).max())
        assert err <= PH.F64_TOL, (k, err)


def test_process_order_is_episodes_sorted_then_windows(g, tmp_path):
  from oatomobile_amd import replay
  L, P, skips = PH.case_params(g, "short")
  written = replay.process(PH.write_raw(g, "short", tmp_path / "raw"), str(tmp_path / "out"), L, P, skips)
  want = []
  for ep in sorted(str(e) for e in g["short_episodes"]):
    tokens, _ = PH.episode_raw(g, "short", ep)
    want += [tokens[i] for i in range(P, len(tokens) - L, skips)]
  assert [os.path.basename(f)[:-4] for f in written] == want and len(want) == 7


def test_short_episode_is_refused_by_name(g, tmp_path):
  from oatomobile_amd import replay
  raw = PH.write_raw(g, "short", tmp_path / "raw")  # epA has 11 samples: one short of 2 + 9 + 1
  os.makedirs(tmp_path / "raw" / "not_an_episode")  # no metadata: skipped, like the reference
  with pytest.raises(ValueError, match="epA"):
    replay.process(raw, str(tmp_path / "out"), future_length=9, past_length=2, num_frame_skips=3)
  with pytest.raises(ValueError, match="epA"):
    replay.pack_episodes(raw, str(tmp_path / "cache"), future_length=9, past_length=2, num_frame_skips=3, goal_stride=3)
  assert len(replay.process(raw, str(tmp_path / "out"), future_length=8, past_length=2, num_frame_skips=3)) == 7


@pytest.mark.parametrize("case,G,stride", [("default", 10, 8), ("short", 10, 3), ("short", 1, 8)])
def test_pack_episodes_equals_pack_cache_of_process(g, tmp_path, case, G, stride):
  """File by file: the six files of pack_cache(process output in that order, targets=True), equal on the numpy path."""
  from oatomobile_amd import replay
  L, P, skips = PH.case_params(g, case)
  raw = PH.write_raw(g, case, tmp_path / "raw")
  files = replay.process(raw, str(tmp_path / "out"), L, P, skips)
  ref = replay.pack_cache(files, str(tmp_path / "ref"), num_goals=G, goal_stride=stride, workers=1, targets=True)
  got = replay.pack_episodes(raw, str(tmp_path / "got"), L, P, skips, num_goals=G, goal_stride=stride)
  assert sorted(os.listdir(tmp_path / "got")) == sorted(os.listdir(tmp_path / "ref")) == sorted(CACHE_FILES)
  assert len(got) == len(ref) == len(files) and got.has_targets
  for name in CACHE_FILES:
    a, b = np.load(tmp_path / "got" / name), np.load(tmp_path / "ref" / name)
    assert a.dtype == b.dtype and a.shape == b.shape, name
    assert a.tobytes() == b.tobytes(), name
  for i in range(len(got)):  # and the BEV comes back bit for bit, -0.0 included
    assert got.lidar(i).tobytes() == replay.load_datum(files[i])["lidar"].tobytes()
  assert any(np.signbit(got.lidar(i)[got.lidar(i) == 0]).any() for i in range(len(got)))


def test_numpy_restatement(g):
  """`_datum.hindsight_targets` is `world2local` per window; mode and goal are `mode_label` / `goal_from_future`; the
  windows that leave the track or cross an episode boundary are NaN; the fixture's labels reach three rungs."""
  from oatomobile_amd import _datum, agents
  modes = set()
  for case in ("default", "short"):
    L, P, skips = PH.case_params(g, case)
    for ep in g["%s_episodes" % case]:
      tokens, raw = PH.episode_raw(g, case, str(ep))
      loc, rot, N = raw["location"], raw["rotation"], len(tokens)
      assert loc.dtype == np.float32 and rot.dtype == np.float32
      frames = np.arange(-1, N + 1)
      future, past = _datum.hindsight_targets(loc, rot, frames, L, P)
      assert future.shape == (N + 2, L, 3) and past.shape == (N + 2, P, 3) and future.dtype == past.dtype == np.float64
      for m, i in enumerate(frames):
        if i - P < 0 or i + L >= N:
          assert np.isnan(future[m]).all() and np.isnan(past[m]).all()
          continue
        kw = dict(current_location=loc[i], current_rotation=rot[i])
        np.testing.assert_array_equal(future[m], agents.world2local(world_locations=loc[i + 1:i + 1 + L], **kw).reshape(L, 3))
        np.testing.assert_array_equal(past[m], agents.world2local(world_locations=loc[i - P:i], **kw).reshape(P, 3))
      ok = np.flatnonzero(~np.isnan(future[:, 0, 0]))
      fxy, goal, mode = _datum.targets_from_future(future[ok], 10, 3)
      for j, m in enumerate(ok):
        f32 = future[m].astype(np.float32)
        assert mode[j] == _datum.mode_label(f32)
        np.testing.assert_array_equal(goal[j], _datum.goal_from_future(f32, 10, 3))
        np.testing.assert_array_equal(fxy[j], f32[:, :2])
        if frames[m] in range(P, N - L, skips):
          modes.add(int(mode[j]))
      # an episode boundary inside the window invalidates it, at either end; one just outside it does not
      i0 = N - L - 1  # the last frame with a full window; row i0 + 1 of `future` (frames starts at -1)
      for lo, hi, valid in ((i0 + L, N, False), (0, i0 - P + 1, False), (0, i0 - P, True)):
        episode = np.zeros(N, np.int32)
        episode[lo:hi] = 7
        f2, p2 = _datum.hindsight_targets(loc, rot, [i0], L, P, episode=episode)
        if valid:
          np.testing.assert_array_equal(f2[0], future[i0 + 1])
          np.testing.assert_array_equal(p2[0], past[i0 + 1])
        else:
          assert np.isnan(f2).all() and np.isnan(p2).all()
  assert modes == {0, 1, 2}  # FORWARD, STOP, LEFT (RIGHT cannot come out of arccos: datasets/carla.py:148-162)


def test_past_length_zero_and_single_step(g):
  """P = 0 (which the reference refuses: tools/make_golden_process.py) and L = 1 keep their [P,3] / [L,3] shapes."""
  from oatomobile_amd import _datum, agents
  _, raw = PH.episode_raw(g, "short", "epB")
  future, past = _datum.hindsight_targets(raw["location"], raw["rotation"], [0, 5], 1, 0)
  assert future.shape == (2, 1, 3) and past.shape == (2, 0, 3)
  np.testing.assert_array_equal(future[1, 0], agents.world2local(current_location=raw["location"][5], current_rotation=raw["rotation"][5],
                                                                 world_locations=raw["location"][6]))


def test_header_and_bindings_agree_on_the_new_entry_points():
  from oatomobile_amd import _lib
  header = open(os.path.join(ROOT, "include", "rip_hip.h")).read()
  sigs = {name: args for name, _, args in _lib.SIGNATURES}
  lib = _lib.load()
  for name in ("rip_hindsight_targets", "rip_code_bev_u8"):
    decl = re.search(r"int %s\(([^;]*)\);" % name, header)
    assert decl is not None, name
    assert len(decl.group(1).split(",")) == len(sigs[name]), name
    assert hasattr(lib, name)
  n = len(set(re.findall(r"\b(rip_[a-z0-9_]+)\s*\(", header)))
  assert n == len(_lib.SIGNATURES)
  for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
    text = open(os.path.join(ROOT, doc)).read()
    quoted = {int(m) for m in re.findall(r"(\d+) (?:`extern \"C\"` )?entry points", text)} - {34, 39, 41, 42}
    assert quoted == {n}, (doc, quoted, n)
  assert lib.rip_abi_version() == 4


def test_entry_points_validate_their_arguments():
  """Argument checks happen before any launch: they run without a GPU."""
  from oatomobile_amd import _lib
  lib = _lib.load()
  p = lambda v=256: _lib.c_void_p(v)  # never dereferenced: every call below is refused
  hs = lambda L=8, P=2, G=10, stride=8, goal=256: lib.rip_hindsight_targets(p(), p(), p(), 20, p(), 3, L, P, G, stride, p(), p(), p(),
                                                                            p(goal), p(), p(), None)
  for kw, word in ((dict(L=0), "L=0"), (dict(P=-1), "P=-1"), (dict(G=0), "G=0"), (dict(G=65), "G=65"), (dict(stride=0), "goal_stride=0"),
                   (dict(L=2, stride=3), "no waypoint")):
    assert hs(**kw) == _lib.RIP_EINVAL
    assert word in lib.rip_last_error().decode(), (kw, lib.rip_last_error())
  code = lambda n: lib.rip_code_bev_u8(p(), 1, 4, 4, 2, p(), n, p(), p(), None)
  for n in (0, 257):
    assert code(n) == _lib.RIP_EINVAL and "n_values" in lib.rip_last_error().decode()
  assert lib.rip_code_bev_u8(p(), 1, 4, 4, 2, p(), 6, p(), p(0), None) == _lib.RIP_EINVAL


def test_raw_dataset_flag(g, tmp_path):
  """`--raw_dataset` parses (default off) and `packed()` takes the raw path: pack_episodes' cache, sources.json listing
  the raw sample files, reused while they are unchanged."""
  import json
  from oatomobile_amd import replay
  from oatomobile_amd.baselines.torch._train_main import SOURCES, packed, parse_args
  base = ["--dataset_dir", str(tmp_path), "--output_dir", str(tmp_path), "--num_epochs", "1"]
  assert parse_args("dim", base).raw_dataset is False
  assert parse_args("cil", base + ["--raw_dataset"]).raw_dataset is True
  split = PH.write_raw(g, "default", tmp_path / "train")
  cache = packed(split, str(tmp_path / "cache"), raw=True)
  assert len(cache) == 3 and cache.has_targets and cache.future.shape == (3, 80, 2)
  ref = replay.pack_episodes(split, str(tmp_path / "ref"))
  for name in CACHE_FILES:
    assert np.load(tmp_path / "cache" / name).tobytes() == np.load(tmp_path / "ref" / name).tobytes(), name
  with open(tmp_path / "cache" / SOURCES) as f:
    assert [s[0] for s in json.load(f)] == sorted(str(t) + ".npz" for t in g["default_ep0_tokens"])
  stamp = os.stat(tmp_path / "cache" / "codes.npy").st_mtime_ns
  assert len(packed(split, str(tmp_path / "cache"), raw=True)) == len(ref)
  assert os.stat(tmp_path / "cache" / "codes.npy").st_mtime_ns == stamp
  with pytest.raises(SystemExit):  # raw episodes are not datum files: the flag is needed
    packed(split, str(tmp_path / "cache2"))
