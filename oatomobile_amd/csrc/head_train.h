// Internal C++ interface of the K-member head step (head_train.hip) behind the rip_head_* entry points of
// include/rip_head.h: the density head (_merger + _decoder) of every ensemble member trained on cached encoder features.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace rip {

// The head = the contiguous tail of arch.packed_spec(): offsets in floats inside one member's [HEAD_NUMEL] vector.
constexpr int HEAD_IN = 133;                        // cat(feat 128, vec 5)
constexpr int H_M0W = 0;                            // _merger._model.0.weight [64,133]
constexpr int H_M0B = H_M0W + 64 * HEAD_IN;         // .0.bias [64]
constexpr int H_M1W = H_M0B + 64;                   // .2.weight [64,64]
constexpr int H_M1B = H_M1W + 64 * 64;
constexpr int H_M2W = H_M1B + 64;                   // .4.weight [64,64]
constexpr int H_M2B = H_M2W + 64 * 64;
constexpr int H_WIH = H_M2B + 64;                   // _decoder._decoder.weight_ih [192,2]
constexpr int H_WHH = H_WIH + 192 * 2;              // weight_hh [192,64]
constexpr int H_BIH = H_WHH + 192 * 64;
constexpr int H_BHH = H_BIH + 192;
constexpr int H_L0W = H_BHH + 192;                  // _decoder._locscale._model.0.weight [32,64]
constexpr int H_L0B = H_L0W + 32 * 64;
constexpr int H_L2W = H_L0B + 32;                   // .2.weight [4,32]
constexpr int H_L2B = H_L2W + 4 * 32;
constexpr int HEAD_NUMEL = H_L2B + 4;               // 32164
static_assert(HEAD_NUMEL == 32164 && HEAD_NUMEL % 4 == 0 && H_M1W % 4 == 0 && H_M2W % 4 == 0 && H_WHH % 4 == 0 &&
              H_L0W % 4 == 0, "float4 loads of a member's head need 16-byte aligned tensors");

// merger records, per (member, row): dz*mask 64 | h2 64 | dh2*mask 64 | h1 64 | dh1*mask 64 | merged 133 | pad 3
constexpr int HEAD_MREC = 456;
constexpr int HM_DZ = 0, HM_H2 = 64, HM_DH2 = 128, HM_H1 = 192, HM_DH1 = 256, HM_IN = 320;

struct HeadArgs {
  const float* head;      // [K][HEAD_NUMEL]
  const float* feat;      // [K][n][128]
  const float* vec;       // [n][5]
  const float* y;         // [K][B][4][2], or nullptr: gathered from `future`
  const float* future;    // [n][L][2]: y = future[row, 0::stride] (+ noise)
  const float* noise;     // [K][B][4][2] or nullptr
  const long long* rows;  // [K][B] indices into the n cache rows, or nullptr: the identity (n == B)
  long long n;
  int K, B, L, stride;
  float* q_rows;          // [K][B]
  float* z;               // [K][B][64] or nullptr
  float* loss;            // [K]
};

size_t head_workspace_bytes(int K, int max_batch);
// Forward (and with grads != nullptr backward) of the K heads on B rows each; `workspace` holds head_workspace_bytes(K, B)
// bytes when grads are wanted.  grads [K][HEAD_NUMEL].  Three launches (two without grads), whatever K and B.
hipError_t launch_head_step(const HeadArgs& a, float* grads, void* workspace, hipStream_t s);

}  // namespace rip
