"""Shared builders for tests (synthetic observations follow SURVEY.md §8(d))."""
import numpy as np


def synth_observation(rng, C=2, G=10, H=200, W=200):
  lidar = (rng.integers(0, 6, size=(H, W, C)) / 5.0) * (rng.random((H, W, C)) < 0.12)
  goal = np.cumsum(np.abs(rng.normal(size=(G, 2))) * 2.0, axis=0)
  goal = np.c_[goal, np.zeros((G, 1))]
  return dict(
      lidar=lidar.astype(np.float32),
      velocity=rng.normal(0, 3.0, size=(3,)).astype(np.float32),
      is_at_traffic_light=np.float32(rng.random() < 0.2),
      traffic_light_state=np.float32(rng.integers(0, 4)),
      goal=goal.astype(np.float32),
  )


# The BEV sizes the shape tests run, (H, W) -> out_hw = 100 unless stated (tests/test_shapes.py, and the CPU pin of the
# reference below in tests/test_host_cpu.py): the last size the LDS-tiled transform takes and the first the generic kernel
# takes, non-square and odd sizes, scale 1, up-sampling (the patch is clipped in every tile), degenerate and narrow inputs.
TRANSFORM_SHAPES = [(200, 200), (208, 208), (209, 209), (208, 120), (120, 208), (199, 201), (100, 100), (64, 48), (1, 5),
                    (5, 1), (1, 1), (207, 3), (400, 100), (160, 240)]
TRANSFORM_CASES = [(h, w, 100) for h, w in TRANSFORM_SHAPES] + [(h, w, o) for h, w in ((200, 200), (64, 48)) for o in (1, 2, 33)]


def _src_coords(size, out):
  """Source rows of one axis as `F.interpolate(align_corners=True)` computes them: the fp32 scale (size-1)/(out-1) (0 when
  out == 1), the fp32 product scale * index, truncated; hi = lo + (lo < size-1); lambda = product - lo in fp32."""
  scale = np.float32(size - 1) / np.float32(out - 1) if out > 1 else np.float32(0.0)
  f = (scale * np.arange(out, dtype=np.float32)).astype(np.float32)
  lo = f.astype(np.int64)
  hi = lo + (lo < size - 1)
  lam = (f - lo.astype(np.float32)).astype(np.float32)
  return lo, hi, lam.astype(np.float64)


def bilinear_swap_ref(x_nchw, out_hw):
  """torch/transforms.py:34-49 in numpy: bilinear [B,C,H,W] -> [B,C,out_hw,out_hw] with align_corners=True, then the H/W
  swap.  The source coordinates are the reference's own (fp32, `_src_coords`: that is its definition — float64
  coordinates sit up to 2e-5 from it); the blend of the four neighbours is float64."""
  x = np.asarray(x_nchw, dtype=np.float64)
  ya, yb, ly = _src_coords(x.shape[2], out_hw)
  xa, xb, lx = _src_coords(x.shape[3], out_hw)
  ly, lx = ly[:, None], lx[None, :]
  top = (1.0 - lx) * x[:, :, ya][:, :, :, xa] + lx * x[:, :, ya][:, :, :, xb]
  bot = (1.0 - lx) * x[:, :, yb][:, :, :, xa] + lx * x[:, :, yb][:, :, :, xb]
  return np.ascontiguousarray(((1.0 - ly) * top + ly * bot).transpose(0, 1, 3, 2))
