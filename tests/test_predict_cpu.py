"""Host side of sample-and-rank prediction (no GPU): the numpy restatement of the device generator against known
answers, the displacement metrics, and the header <-> `_lib.SIGNATURES` agreement of the two new entry points."""

import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (counter, key) -> words: the Random123 known answers of Philox4x32-10 (zeros, all ones, digits of pi)
KNOWN_WORDS = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]
# seed 2024: sample id -> x[0..7]
KNOWN_NORMALS = {
    0: [-0.11691724, 0.99785749, 0.15243754, 0.08834561, -1.05520091, -1.14492148, 0.53078726, 1.14905974],
    2**32 + 5: [0.61690571, 0.86306567, -0.27411423, -0.54956671, -0.03821556, 0.21167508, -0.14071117, 1.28665505],
}
# float32 Box-Muller through different libms: a few ulp of values up to 5.77 (ulp 4.8e-7); the table has 8 decimals
NORMAL_ATOL = 1e-6


def test_philox_words_known_answers():
  from oatomobile_amd import prediction
  for counter, key, want in KNOWN_WORDS:
    got = prediction.philox4x32(np.array(counter, np.uint32), np.array(key, np.uint32))
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert " ".join("%08x" % w for w in got) == want
  # batched, and the counter / key layout philox_normal uses: (g lo, g hi, c, 0); (seed lo, seed hi)
  counters = np.array([c for c, _, _ in KNOWN_WORDS], np.uint32)
  keys = np.array([k for _, k, _ in KNOWN_WORDS], np.uint32)
  got = prediction.philox4x32(counters, keys)
  assert [" ".join("%08x" % w for w in row) for row in got] == [w for _, _, w in KNOWN_WORDS]


def test_philox_normal_known_answers():
  from oatomobile_amd import philox_normal
  for g, want in KNOWN_NORMALS.items():
    got = philox_normal(2024, g, 1)
    assert got.shape == (1, 8) and got.dtype == np.float32
    np.testing.assert_allclose(got[0], want, rtol=0, atol=NORMAL_ATOL)
  # a sample is a function of (seed, id) alone: any window over the ids gives the same rows
  a = philox_normal(2024, 2**32 - 3, 12)
  np.testing.assert_array_equal(a[3:9], philox_normal(2024, 2**32, 6))
  np.testing.assert_array_equal(a[8], philox_normal(2024, 2**32 + 5, 1)[0])
  assert not np.array_equal(philox_normal(2025, 0, 1), philox_normal(2024, 0, 1))
  assert not np.array_equal(philox_normal(2024 + 2**32, 0, 1), philox_normal(2024, 0, 1))  # the key's high word counts
  assert philox_normal(1, 0, 0).shape == (0, 8)
  with pytest.raises(ValueError):
    philox_normal(-1, 0, 1)


def test_philox_normal_moments():
  """65 536 x 8 standard normals, every moment within 5 sigma: the mean of n = 524 288 values (sigma 1 / sqrt(n):
  5 sigma = 0.0069), their variance (sigma sqrt(2 / n): 0.0098), the 8 column means (sigma 1 / 256: 0.0195) and the 28
  correlations between columns (sigma 1 / 256: 0.0195).  Measured: 0.0004, 0.0009, 0.0062, 0.0118."""
  from oatomobile_amd import philox_normal
  x = philox_normal(2024, 0, 65536).astype(np.float64)
  assert np.isfinite(x).all() and np.abs(x).max() <= 5.77
  corr = np.corrcoef(x.T)
  got = (abs(x.mean()), abs(x.var() - 1.0), np.abs(x.mean(0)).max(), np.abs(corr - np.eye(8)).max())
  print("philox_normal moments: mean %.4f variance %.4f column means %.4f correlations %.4f" % got)
  assert got[0] <= 0.0069
  assert got[1] <= 0.0098
  assert got[2] <= 0.0195
  assert got[3] <= 0.0195


def test_displacement_errors_and_min_over_k():
  from oatomobile_amd import displacement_errors, min_over_k
  target = np.array([[0, 0], [1, 0], [2, 0], [3, 0]], np.float32)
  y = np.stack([target + np.array([3, 4], np.float32),                     # 5 away at every step
                target,                                                   # the target itself
                target + np.array([[0, 0], [0, 1], [0, 2], [0, 3]], np.float32)])  # 0, 1, 2, 3 away
  ade, fde = displacement_errors(y, target)
  assert ade.dtype == np.float64 and ade.shape == (3,)
  np.testing.assert_allclose(ade, [5.0, 0.0, 1.5], rtol=0, atol=1e-12)
  np.testing.assert_allclose(fde, [5.0, 0.0, 3.0], rtol=0, atol=1e-12)
  # batched: [B,k,T,2] against [B,T,2]
  ade2, fde2 = displacement_errors(np.stack([y, y[::-1]]), np.stack([target, target]))
  np.testing.assert_allclose(ade2, [[5.0, 0.0, 1.5], [1.5, 0.0, 5.0]], rtol=0, atol=1e-12)
  np.testing.assert_allclose(fde2, [[5.0, 0.0, 3.0], [3.0, 0.0, 5.0]], rtol=0, atol=1e-12)
  np.testing.assert_array_equal(min_over_k(ade2, 1), [5.0, 1.5])
  np.testing.assert_array_equal(min_over_k(ade2, 2), [0.0, 0.0])
  np.testing.assert_array_equal(min_over_k(np.array([3.0, 2.0, 1.0]), 2), 2.0)
  for k in (0, 4):
    with pytest.raises(ValueError):
      min_over_k(ade2, k)
  with pytest.raises(ValueError):
    displacement_errors(y, target[:3])


def test_prediction_exports():
  import oatomobile_amd as P
  for name in ("Prediction", "philox_normal", "displacement_errors", "min_over_k"):
    assert name in P.__all__ and hasattr(P, name)
  assert P.Prediction._fields == ("y", "loss", "index", "member", "ade", "fde")
  assert callable(P.RIPAgent.predict_batch) and callable(P.RIPAgent.predict_batch_coded)
  from oatomobile_amd import replay
  assert callable(replay.predict_cache)


def test_header_and_signatures_agree_on_the_new_symbols():
  """`rip_sample_normal` and `rip_predict`: declared in include/rip_hip.h, bound in `_lib.SIGNATURES` with as many
  arguments as the declaration has (64-bit seed, ids and row0 as 64-bit ctypes), exported by the library; the ABI
  version stays 4."""
  import ctypes
  from oatomobile_amd import _lib
  header = open(os.path.join(ROOT, "include", "rip_hip.h")).read()
  sigs = {name: (res, args) for name, res, args in _lib.SIGNATURES}
  for name in ("rip_sample_normal", "rip_predict"):
    m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
    assert m, name
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = sigs[name]
    assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
    for p, a in zip(params, args):
      if "*" in p or p.startswith("rip_stream_t"):
        assert a is ctypes.c_void_p, (name, p)
      elif p.startswith("uint64_t"):
        assert a is ctypes.c_uint64, (name, p)
      elif p.startswith("int64_t"):
        assert a is ctypes.c_int64, (name, p)
      elif p.startswith("float"):
        assert a is ctypes.c_float, (name, p)
      else:
        assert p.startswith("int ") and a is ctypes.c_int, (name, p)
    assert hasattr(_lib.load(), name)
  assert _lib.load().rip_abi_version() == _lib.ABI_VERSION == 4
