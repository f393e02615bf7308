"""Host side of the ensemble-disagreement feature: `detection_auroc` and the package-root exports (no GPU)."""

import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force_auroc(a, b):
  wins = sum(1.0 if y > x else (0.5 if y == x else 0.0) for x in a for y in b)
  return wins / (len(a) * len(b))


def test_detection_auroc_against_a_pair_count():
  from oatomobile_amd import detection_auroc
  rng = np.random.default_rng(12)
  for n_in, n_out in ((1, 1), (7, 5), (40, 61)):
    a = rng.integers(0, 9, size=n_in) / 4.0          # few levels: many ties
    b = rng.integers(2, 12, size=n_out) / 4.0
    got = detection_auroc(a, b)
    assert isinstance(got, float)
    assert got == pytest.approx(brute_force_auroc(a, b), abs=1e-12)
    assert detection_auroc(b, a) == pytest.approx(1.0 - got, abs=1e-12)
  a, b = rng.normal(size=(6, 5)), rng.normal(0.5, 1.0, size=33).astype(np.float32)  # any shape / float dtype
  assert detection_auroc(a, b) == pytest.approx(brute_force_auroc(a.ravel(), b), abs=1e-12)


def test_detection_auroc_limits():
  from oatomobile_amd import detection_auroc
  assert detection_auroc([0.1, 0.2, 0.3], [0.4, 5.0]) == 1.0
  assert detection_auroc([0.4, 5.0], [0.1, 0.2, 0.3]) == 0.0
  x = [3.0, 1.0, 2.0, 2.0]
  assert detection_auroc(x, x) == 0.5
  for a, b in (([], [1.0]), ([1.0], []), ([], [])):
    with pytest.raises(ValueError, match="non-empty"):
      detection_auroc(a, b)


def test_plan_stats_exports_do_not_load_the_library():
  """`PlanStats` and `detection_auroc` come from the package root; importing and using them does not dlopen
  librip_hip.so (a fresh interpreter: this process may have loaded it for another test)."""
  code = ("import oatomobile_amd as P, numpy as np\n"
          "from oatomobile_amd import PlanStats, detection_auroc, _lib\n"
          "s = PlanStats(q=np.zeros((2, 1)), mean=np.zeros(1), variance=np.ones(1), min=np.zeros(1), max=np.zeros(1))\n"
          "assert s._fields == ('q', 'mean', 'variance', 'min', 'max') and s.variance[0] == 1 and s[1] is s.mean\n"
          "assert detection_auroc([0.0], [1.0]) == 1.0\n"
          "assert 'PlanStats' in P.__all__ and 'detection_auroc' in P.__all__\n"
          "assert _lib._lib is None, 'the library was loaded'\n"
          "print('ok')\n")
  r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
  assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
