// xpt_dwstage.h -- what the fused depthwise stages share: xpt_mbconv.hip (MobileNetV2: 3x3 -> BatchNorm -> ReLU6) and
// xpt_effconv.hip (EfficientNet: k x k -> BatchNorm -> swish -> squeeze-and-excite).  Included by those two files only.
//
// Activations NHWC in the 16-bit format of the build.  A lane owns 8 channels (16 bytes) of a pixel; every gathered activation
// access is one 16-byte buffer load whose range check supplies the zeros of the halo (the offset marker DW_OOB past the buffer:
// no per-tap branch, no mask arithmetic on the values).
//
// Every kernel that sums over pixels (the parameter gradients of both backwards, the pool and dL/dgate of the EfficientNet
// stage) uses ONE plan: a workgroup owns a chunk of output rows of ONE image and a block of channel groups, its lanes walk the
// chunk's pixels, the workgroup adds them through LDS in lane order and writes one row of a partial matrix; rows are added in
// row order by whoever finishes them.  No atomics, so a captured step replays bit for bit.
#pragma once
#include "xpt_common.h"

namespace {

typedef unsigned int dw_u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned DW_OOB = 0x80000000u;        // byte offset no buffer of < 2^31 bytes contains: the load returns zeros
constexpr int DW_PASS = 4;                      // entries per LDS pass of a backward's workgroup sum

struct DwDims {
  int B, H, W, C, OH, OW, pad_t, pad_l;
};

struct DwPlan {
  int rpc;       // output rows per chunk
  int cpi;       // chunks per image
  int chunks;    // B * cpi: rows of a partial matrix
  int cgb;       // channel groups per workgroup (a divisor of C / 8, at most the cap given to dw_plan)
  int ncb;       // channel blocks: (C / 8) / cgb
};

__device__ __forceinline__ void dw_unpack(const dw_u32x4& v, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = xpt_h2f_lo(v[i]);
    f[2 * i + 1] = xpt_h2f_hi(v[i]);
  }
}

__device__ __forceinline__ uint4 dw_pack(const float (&f)[8]) {
  unsigned p[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = (unsigned)xpt_f2h(f[2 * i]) | ((unsigned)xpt_f2h(f[2 * i + 1]) << 16);
  return make_uint4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ dw_u32x4 dw_load16(const void* p, size_t element) {
  const uint4 v = *(const uint4*)((const unsigned short*)p + element);
  return dw_u32x4{v.x, v.y, v.z, v.w};
}

__device__ __forceinline__ void dw_load8f(const float* p, float (&f)[8]) {
  const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1];
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// first input row of the chunk that starts at output row oy: the chunks of an image tile its input rows [0, H)
__device__ __forceinline__ int dw_in_row(int oy, int S, int OH, int H) {
  return oy <= 0 ? 0 : (oy >= OH ? H : min(H, oy * S));
}

bool dw_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int dw_check(const DwDims& d, int k, int stride) {
  if (d.B <= 0 || d.H <= 0 || d.W <= 0 || d.C <= 0 || d.OH <= 0 || d.OW <= 0) return XPT_ERR_SHAPE;
  if (d.C % 8 != 0) return XPT_ERR_ARG;                                  // 16-byte channel groups
  if (k != 3 && k != 5) return XPT_ERR_ARG;
  if (stride != 1 && stride != 2) return XPT_ERR_ARG;
  if (d.pad_t < 0 || d.pad_t > k / 2 || d.pad_l < 0 || d.pad_l > k / 2) return XPT_ERR_ARG;
  // the centre of every window inside the input (SAME padding of an odd window, either stride, any parity)
  if ((long long)(d.OH - 1) * stride + k / 2 - d.pad_t > d.H - 1 || (long long)(d.OW - 1) * stride + k / 2 - d.pad_l > d.W - 1)
    return XPT_ERR_SHAPE;
  // 32-bit byte offsets below the out-of-range marker, 32-bit item numbers
  if ((long long)d.B * d.H * d.W * d.C * 2 >= (1LL << 31) || (long long)d.B * d.OH * d.OW * d.C * 2 >= (1LL << 31))
    return XPT_ERR_SHAPE;
  return XPT_OK;
}

// the row-chunk plan of a map; max_cgb: channel groups per workgroup at most (first of all it keeps the workgroup count up)
DwPlan dw_plan(int B, int OH, int OW, int C, int max_cgb) {
  DwPlan p;
  const int CG = C / 8;
  int cgb = 1;
  for (int dv = 1; dv <= max_cgb && dv <= CG; ++dv)
    if (CG % dv == 0) cgb = dv;
  auto groups = [&](int rpc, int g) { return (long long)B * ((OH + rpc - 1) / rpc) * (CG / g); };
  int rpc = 1;
  while (rpc < OH && groups(rpc, cgb) > 2048) rpc *= 2;
  // few workgroups (the 1/16 and 1/32 maps): spread over channel groups, down to one lane row per output pixel of the chunk
  while (cgb > 1 && groups(rpc, cgb) < 512 && 256 / cgb < rpc * OW) {
    int next = cgb - 1;
    while (CG % next != 0) --next;
    cgb = next;
  }
  p.rpc = rpc;
  p.cpi = (OH + rpc - 1) / rpc;
  p.chunks = B * p.cpi;
  p.cgb = cgb;
  p.ncb = CG / cgb;
  return p;
}

}  // namespace
