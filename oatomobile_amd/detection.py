"""Scoring a disagreement statistic as a detector of distribution shift (plain numpy, no device)."""

import numpy as np


def detection_auroc(scores_in, scores_out) -> float:
  """Area under the ROC curve of a score that should be HIGHER on shifted scenes (e.g. `PlanStats.variance`): the
  probability that a scene drawn from `scores_out` (shifted) gets a higher score than one drawn from `scores_in`
  (in-distribution), ties counting one half.  1.0 = separated, 0.5 = uninformative.  ValueError on an empty side."""
  a = np.asarray(scores_in, dtype=np.float64).ravel()
  b = np.asarray(scores_out, dtype=np.float64).ravel()
  if a.size == 0 or b.size == 0:
    raise ValueError("detection_auroc: both score sets must be non-empty (got %d in-distribution, %d shifted)" %
                     (a.size, b.size))
  a = np.sort(a)
  below = np.searchsorted(a, b, side="left")           # in-distribution scores strictly below each shifted score
  ties = np.searchsorted(a, b, side="right") - below   # ... equal to it
  return float((below.sum() + 0.5 * ties.sum()) / (a.size * b.size))
