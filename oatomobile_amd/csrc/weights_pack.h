// Internal C++ interface between the C ABI (rip_abi.hip) and the on-device weight packers (weights_pack.hip):
// rip_load_model's host work (fold_and_pack, pack_split_tiles, pack_split_rows, pack_split_operands) as four launches on
// a stream, reading one member's packed parameter vector from device memory and writing the eight weight buffers of a
// handle slot in place.  The host packers are the reference: every byte must equal theirs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "encoder.h"

namespace rip {

// one contiguous run of the packed vector: a conv (weights + BatchNorm) or a plain copy (classifier, merger)
struct FoldSeg {
  unsigned src;      // first float of the run in the packed vector
  unsigned wn;       // conv: weight elements; copy: floats
  unsigned per_out;  // conv: weights per output channel
  unsigned cin, cout;
  unsigned kind;     // LayerKind, or PK_COPY
  unsigned w_off, b_off;  // blob offsets (copy: w_off = destination)
};
constexpr unsigned PK_COPY = 3;
constexpr int PK_MAX_SEG = 64;
struct FoldPlan {
  int n_seg = 0;
  unsigned start[PK_MAX_SEG + 1];  // work items before segment i (a conv has wn + cout: weights, then biases)
  FoldSeg seg[PK_MAX_SEG];
};

// operand records of the fp32 encoder's split-f16 blocks (encoder_split_tile.hip / encoder_split_rows.hip)
struct TileBlk {
  unsigned off, rec, nch;  // first half of the block's records, halves per chunk record, chunks
  unsigned cin, hid, ksx, nfe, nfp;
  unsigned we_off, wp_off, wd_off, bd_off, be_off;
};
struct RowsBlk {
  unsigned off, n;  // first half, halves
  unsigned cin, hid, cout, nfe, nkp;
  unsigned we_off, wp_off;
};
struct OperandPlan {
  int n_tile = 0, n_rows = 0, has_head = 0;
  unsigned head_off = 0, head_w_off = 0, head_b_off = 0;
  unsigned tiles_total = 0, rows_total = 0;
  TileBlk tile[12];
  RowsBlk rows[8];
};

struct PackPlan {
  bool ok = false;       // false: the plan's layouts are not the ones this file re-derives (a load is refused)
  size_t numel = 0;      // floats of a packed parameter vector
  size_t flow_pos = 0;   // first float of the flow tensors in it
  FoldPlan fold;
  OperandPlan ops;
};
PackPlan build_pack_plan(const EncoderPlan& plan);

// slot k of the handle's buffers (pointers to the slot's first element) and four zero-able device words:
// flags[0] = bits of max |w| over the finite flow weights, flags[1] = a flow weight is NaN / infinite,
// flags[2] = a folded pointwise weight is not below SPLIT_ENC_W_LIMIT
struct PackTargets {
  float* enc_w;
  unsigned short* enc_wh;
  float* enc_wt;
  unsigned short* enc_wc;
  unsigned short* enc_wr;
  float* flow_w;
  float* mfma_w;
  uint32_t* split_w;
  unsigned* flags;
};
hipError_t launch_pack_weights(const EncoderPlan& plan, const PackPlan& pp, const float* packed_dev, const PackTargets& t,
                               hipStream_t s);

}  // namespace rip
