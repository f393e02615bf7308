"""Float64 restatement of the head step (`rip_head_forward_backward`, `train.HeadTrainer`) for tests/test_head_train*.py:
the merger and `oracle.reference_cpu.flow_inverse` on an `OracleImitativeModel(...).double()` with torch autograd, and
the fixed cases (weights, features, targets) both test files build from seeds alone, so that the CPU file can assert the
ReLU-kink condition of exactly the inputs the GPU file runs."""

import functools

import numpy as np
import torch

from oatomobile_amd import arch
from oatomobile_amd import weights as W
from oracle import reference_cpu as O

HEAD_SPEC = [(k, s) for k, s in arch.packed_spec() if not k.startswith("_encoder.")]  # merger.0/2/4 weight + bias, GRU weight_ih / weight_hh / bias_ih / bias_hh, locscale 0 and 2
HEAD_KEYS = [k for k, _ in HEAD_SPEC]
HEAD_NUMEL = sum(int(np.prod(s)) for _, s in HEAD_SPEC)
LEARNING_MARGIN = 1.6e-7  # tests/test_head_train_cpu.py measures it; the GPU learning test's bound is ten times this
KINK_MARGIN = 1e-4  # smallest |pre-activation| a case may have: no ReLU decision can differ between fp32 and float64


def unpack_head(vector):
  """One member's packed head [HEAD_NUMEL] (numpy) -> {state_dict key: array}."""
  out, pos = {}, 0
  for key, shape in HEAD_SPEC:
    n = int(np.prod(shape))
    out[key] = np.asarray(vector[pos:pos + n]).reshape(shape)
    pos += n
  assert pos == len(vector) == HEAD_NUMEL
  return out


def pack_head(state_dict):
  return np.concatenate([np.asarray(state_dict[k], np.float32).reshape(-1) for k in HEAD_KEYS])


def head_model(head_vector, dtype=torch.float64):
  """An oracle model whose head is `head_vector` (its encoder is left as constructed: nothing here runs it)."""
  m = O.OracleImitativeModel()
  head = unpack_head(np.asarray(head_vector, np.float32))
  res = m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in head.items()}, strict=False)
  assert not res.unexpected_keys and all(k.startswith("_encoder.") for k in res.missing_keys)
  return m.to(dtype)


def head_params(model):
  named = dict(model.named_parameters())
  return [named[k] for k in HEAD_KEYS]


def head_ref(model, feat, vec, y):
  """loss = -mean_b(log_prob - logabsdet) of one member in the model's own dtype and its gradient for every head tensor.
  feat [B,128], vec [B,5], y [B,4,2] (numpy or tensors).  -> dict(q_rows [B], loss, z [B,64], grads {key: array},
  min_pre = the smallest |pre-activation| over the merger's three layers and the flow head's a1 of all four steps)."""
  dt = next(model.parameters()).dtype
  feat, vec, y = (torch.as_tensor(np.asarray(t), dtype=dt) for t in (feat, vec, y))
  ps = head_params(model)
  was = [p.requires_grad for p in ps]
  for p in ps:
    p.requires_grad_(True)
  x = torch.cat([feat, vec], dim=-1)
  min_pre = float("inf")
  for layer in model._merger._model:
    x = layer(x)
    if isinstance(layer, torch.nn.Linear):
      min_pre = min(min_pre, float(x.detach().abs().min()))
  z = x
  _, log_prob, lad = O.flow_inverse(model, y, z)
  q = log_prob - lad
  loss = -q.mean()
  grads = torch.autograd.grad(loss, ps)
  with torch.no_grad():  # the flow head's pre-ReLU a1 of every step (teacher-forced hidden states)
    h, u = z.detach(), torch.zeros(y.shape[0], 2, dtype=dt)
    for t in range(y.shape[1]):
      h = O._gru_step(model._decoder, u, h)
      min_pre = min(min_pre, float(model._decoder._locscale._model[0](h).abs().min()))
      u = y[:, t, :]
  for p, w in zip(ps, was):
    p.requires_grad_(w)
  return dict(q_rows=q.detach().numpy(), loss=float(loss.detach()), z=z.detach().numpy(),
              grads={k: g.numpy() for k, g in zip(HEAD_KEYS, grads)}, min_pre=min_pre)


# ------------------------------------------------------------------------------------------------
# the fixed cases
# ------------------------------------------------------------------------------------------------
FEAT_SCALE = 2.0     # synthetic features ~ N(0, FEAT_SCALE^2): the synthetic encoders' logits on random BEVs have a standard deviation of 2.1
MEMBER_SEEDS = (211, 212, 213)  # distinct synthetic weights per member
DEAD_UNIT = 7        # merger layer-0 unit of member 0 that the (K=3, B=5) case kills on every row (bias -50)
# (K, B) -> data seed, chosen so that head_ref's min_pre >= KINK_MARGIN for every member (asserted by the CPU test)
CASE_SEEDS = {(1, 1): 0, (1, 5): 0, (1, 67): 9, (3, 1): 0, (3, 5): 0, (3, 67): 193}


@functools.lru_cache(maxsize=None)
def _member_head(seed):
  return W.pack_state_dict(W.synthetic_state_dict(seed))[-HEAD_NUMEL:].astype(np.float32)


def case_heads(K, dead=False):
  heads = np.stack([_member_head(s) for s in MEMBER_SEEDS[:K]])
  if dead:
    heads[0, 64 * 133 + DEAD_UNIT] = -50.0
  return heads


def case_vec(rng, B):
  return np.concatenate([rng.normal(0, 3.0, (B, 3)), (rng.random((B, 1)) < 0.2), rng.integers(0, 4, (B, 1))], axis=1).astype(np.float32)


def case_targets(rng, K, B):
  """Plan-scale targets (a few metres, increasing along the trajectory); the last row of member 0 is far off: about
  100 - 150 m, where the base-space |x| is in the tens and q about -2e4.  Not farther: dW_ih sums d(gate) * y_prev, and a
  saturating tanh stored in fp32 leaves 1 - n^2 with an absolute error of one ulp of 1, which the far row multiplies by
  its |dh| * |y_prev|.  At 300 - 450 m torch's own fp32 autograd is 8e-5 off float64 on that tensor in the metric of the
  GPU tests, which would leave their 1e-4 bound to chance; the CPU test asserts that at this distance it stays below 1e-5,
  a tenth of the bound."""
  y = np.cumsum(np.abs(rng.normal(size=(K, B, 4, 2))) * 1.5, axis=2)
  y[0, B - 1] = y[0, B - 1] * 10.0 + 100.0
  return y.astype(np.float32)


def make_case(K, B, seed=None):
  """The synthetic parity case (K, B): heads [K,P], feat [K,B,128], vec [B,5], y [K,B,4,2], float32 numpy."""
  rng = np.random.default_rng(1000 * K + B + 100000 * (CASE_SEEDS[(K, B)] if seed is None else seed))
  feat = (FEAT_SCALE * rng.standard_normal((K, B, 128))).astype(np.float32)
  return dict(heads=case_heads(K, dead=(K, B) == (3, 5)), feat=feat, vec=case_vec(rng, B), y=case_targets(rng, K, B))


REAL_K, REAL_B, REAL_SEED = 3, 5, 6


def real_case_inputs(seed=None):
  """The real-feature parity case: lidar [5,200,200,2] random BEVs (tests.helpers.synth_observation), vec [5,5],
  y [3,5,4,2] and the heads [3,P]; the features are the agent's own (`RIPAgent.features_batch`) on these BEVs."""
  from tests.helpers import synth_observation
  rng = np.random.default_rng(9000 + (REAL_SEED if seed is None else seed))
  lidar = np.stack([synth_observation(rng)["lidar"] for _ in range(REAL_B)])
  return dict(heads=case_heads(REAL_K), lidar=lidar, vec=case_vec(rng, REAL_B), y=case_targets(rng, REAL_K, REAL_B))


LEARN_K, LEARN_ROWS, LEARN_STEPS, LEARN_LR, LEARN_NOISE = 2, 64, 40, 1e-3, 1e-2


def learning_case():
  """The learning test's data: heads [2,P], feat [2,64,128], vec [64,5], target [64,4,2] (per observation, shared by the
  members) and the per-step target noise [40,2,64,4,2], from a fixed generator."""
  rng = np.random.default_rng(4242)
  feat = (FEAT_SCALE * rng.standard_normal((LEARN_K, LEARN_ROWS, 128))).astype(np.float32)
  vec = case_vec(rng, LEARN_ROWS)
  target = np.cumsum(np.abs(rng.normal(size=(LEARN_ROWS, 4, 2))) * 1.5, axis=1).astype(np.float32)
  noise = (LEARN_NOISE * rng.standard_normal((LEARN_STEPS, LEARN_K, LEARN_ROWS, 4, 2))).astype(np.float32)
  return dict(heads=case_heads(LEARN_K), feat=feat, vec=vec, target=target, noise=noise)


def learning_curve(case, dtype):
  """The losses [steps, K] of `LEARN_STEPS` Adam steps (torch.optim.Adam, lr `LEARN_LR`) on the case in `dtype`: loss k of
  step s is evaluated before the step, on target + noise[s, k]."""
  K = case["heads"].shape[0]
  curve = np.zeros((LEARN_STEPS, K))
  for k in range(K):
    model = head_model(case["heads"][k], dtype)
    ps = head_params(model)
    for p in ps:
      p.requires_grad_(True)
    opt = torch.optim.Adam(ps, lr=LEARN_LR)
    for s in range(LEARN_STEPS):
      y = case["target"] + case["noise"][s, k]
      r = head_ref(model, case["feat"][k], case["vec"], y)
      for p, key in zip(ps, HEAD_KEYS):
        p.grad = torch.as_tensor(r["grads"][key]).clone()
      opt.step()
      curve[s, k] = r["loss"]
  return curve


def case_min_pre(case):
  """The smallest |pre-activation| of a case over its members (float64)."""
  K = case["heads"].shape[0]
  return min(head_ref(head_model(case["heads"][k]), case["feat"][k], case["vec"], case["y"][k])["min_pre"] for k in range(K))
