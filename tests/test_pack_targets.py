"""CPU tests of the training targets in the packed replay cache (`replay.pack_cache(..., targets=True)`) and of the
target downsampling check used by `replay.DeviceCache.batch`.  No GPU needed."""
import os

import numpy as np
import pytest

from tests.helpers import synth_observation


def _datums(tmp_path, n, C=2, L=80, seed=0):
  from oatomobile_amd import replay
  ep = replay.Episode(str(tmp_path), "ep")
  rng = np.random.default_rng(seed)
  for i in range(n):
    o = synth_observation(np.random.default_rng(100 + i), C=C)
    # every driving mode: short futures are STOP, the turn direction from the heading of the last waypoint
    heading = rng.choice([0.0, 0.5, -0.5, 1.2])
    scale = 0.01 if i % 5 == 0 else 0.5
    steps = np.abs(rng.normal(size=(L, 1))) * scale
    fut = np.concatenate([np.cumsum(steps * np.cos(heading), 0), np.cumsum(steps * np.sin(heading), 0),
                          rng.normal(size=(L, 1))], axis=1).astype(np.float32)
    ep.append("d%03d" % i, lidar=o["lidar"], velocity=o["velocity"], is_at_traffic_light=o["is_at_traffic_light"],
              traffic_light_state=o["traffic_light_state"], player_future=fut)
  return ep.files()


@pytest.mark.parametrize("workers", [1, 3])
def test_pack_targets_equal_load_datum(tmp_path, workers):
  from oatomobile_amd import replay
  files = _datums(tmp_path, 23)
  cache = replay.pack_cache(files, str(tmp_path / "cache"), chunk=4, workers=workers, targets=True)
  assert cache.has_targets
  assert cache.future.shape == (23, 80, 2) and cache.future.dtype == np.float32
  assert cache.mode.shape == (23,) and cache.mode.dtype == np.float32
  for i, f in enumerate(files):
    d = replay.load_datum(f, mode=True)
    np.testing.assert_array_equal(cache.future[i], d["player_future"][:, :2])
    assert cache.mode[i] == d["mode"][0]  # the label as the datum says: STOP (1) is kept
    np.testing.assert_array_equal(cache.lidar(i), d["lidar"])
  assert {0.0, 1.0} <= set(np.unique(cache.mode).tolist())
  assert len(set(np.unique(cache.mode).tolist())) >= 3


def test_pack_without_targets_is_unchanged(tmp_path):
  from oatomobile_amd import replay
  files = _datums(tmp_path, 9)
  a = replay.pack_cache(files, str(tmp_path / "plain"), chunk=4, workers=2)
  assert sorted(os.listdir(tmp_path / "plain")) == sorted(replay.CACHE_FILES)
  assert not a.has_targets and a.future is None and a.mode is None
  b = replay.pack_cache(files, str(tmp_path / "full"), chunk=4, workers=2, targets=True)
  assert sorted(os.listdir(tmp_path / "full")) == sorted(replay.CACHE_FILES + ("future.npy", "mode.npy"))
  for name in replay.CACHE_FILES:  # the four files themselves do not depend on `targets`
    with open(tmp_path / "plain" / name, "rb") as f1, open(tmp_path / "full" / name, "rb") as f2:
      assert f1.read() == f2.read(), name


@pytest.mark.parametrize("L,T,stride", [(80, 4, 20), (80, 40, 2), (80, 80, 1), (80, 1, 80), (9, 3, 3)])
def test_downsample_stride(L, T, stride):
  from oatomobile_amd import replay
  assert replay.downsample_stride(L, T) == stride
  assert len(range(0, L, stride)) == T


@pytest.mark.parametrize("L,T", [(80, 3), (80, 7), (80, 0), (80, 81), (10, 3)])
def test_downsample_stride_refuses_a_slice_of_another_length(L, T):
  from oatomobile_amd import replay
  with pytest.raises(ValueError):
    replay.downsample_stride(L, T)


def test_device_cache_refuses_a_cache_without_targets(tmp_path):
  from oatomobile_amd import replay
  files = _datums(tmp_path, 3)
  cache = replay.pack_cache(files, str(tmp_path / "plain"), workers=1)
  with pytest.raises(ValueError, match="targets=True"):
    replay.DeviceCache(cache, "cuda:0")


def test_cli_refuses_a_dim_horizon_other_than_four(tmp_path):
  from oatomobile_amd.baselines.torch._train_main import parse_args
  with pytest.raises(SystemExit):
    parse_args("dim", ["--dataset_dir", str(tmp_path), "--output_dir", str(tmp_path), "--num_epochs", "1",
                       "--num_timesteps_to_keep", "8"])
  args = parse_args("cil", ["--dataset_dir", str(tmp_path), "--output_dir", str(tmp_path), "--num_epochs", "1",
                            "--num_timesteps_to_keep", "8"])
  assert args.num_timesteps_to_keep == 8 and args.batch_size == 512 and args.save_model_frequency == 4
  assert args.learning_rate == 1e-3 and args.weight_decay == 0.0 and not args.clip_gradients


def test_cli_repacks_when_the_datum_files_change(tmp_path):
  """The command line reuses a packed cache only for the datum files it was packed from: a file rewritten with other
  content (same file count) repacks it."""
  from oatomobile_amd import replay
  from oatomobile_amd.baselines.torch._train_main import packed
  files = _datums(tmp_path, 6)
  split = os.path.dirname(files[0])
  cache_dir = str(tmp_path / "cache")
  first = packed(split, cache_dir)
  stamp = os.stat(os.path.join(cache_dir, "codes.npy")).st_mtime_ns
  again = packed(split, cache_dir)  # unchanged files: reused, not repacked
  assert os.stat(os.path.join(cache_dir, "codes.npy")).st_mtime_ns == stamp
  before = np.array(first.future)  # a copy: the memmap would see the repacked file
  np.testing.assert_array_equal(np.asarray(again.future), before)
  d = replay.load_datum(files[2])
  fut = d["player_future"] + 5.0
  os.remove(files[2])
  np.savez_compressed(files[2], lidar=d["lidar"], velocity=d["velocity"], is_at_traffic_light=d["is_at_traffic_light"],
                      traffic_light_state=d["traffic_light_state"], player_future=fut)
  fresh = packed(split, cache_dir)
  np.testing.assert_array_equal(np.asarray(fresh.future[2]), fut[:, :2])
  for i in (0, 1, 3, 4, 5):
    np.testing.assert_array_equal(np.asarray(fresh.future[i]), before[i])
