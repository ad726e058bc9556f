// xpt_resnet.hip -- what ResNet50V2 (keras resnet_v2.ResNet50V2, block2 / stack2) adds to the encoder kernels.
//
// 1. Residual junction, forward, ONE launch: `<name>_3_conv` (1x1, bias) + the shortcut add `<name>_out` + the NEXT block's
//    `_preact_bn` / `_preact_relu` (or `post_bn` / `post_relu` after the last block):
//        out[m, n] = sum_k h[m, k] W3[n, k] + b3[n] + shortcut[src(m), n]          (stored in the 16-bit format)
//        pre[m, n] = relu(out[m, n] * s[n] + t[n]),   s = gamma rsqrt(var + eps),  t = beta - mean s
//    shortcut is one of: the block input itself (src(m) = m), the block input at pixel (2 oy, 2 ox) (what
//    MaxPooling2D(1, strides=2) selects: the last block of a stack), or `<name>_0_conv` of the pre-activated input, computed
//    by the SAME wave as a second GEMM into the same accumulator (out = h W3^T + preact W0^T + b3 + b0).
//    GEMM view as in xpt_conv.hip: A = weight rows, B = pixel rows, both k-contiguous -- the operand layout of
//    v_mfma_f32_32x32x16: one 16-byte load per fragment, no LDS.  A wave owns 32 channels x 32 pixels; a lane's accumulator
//    is 4 groups of 4 CONSECUTIVE channels of one pixel, so the whole epilogue stays in registers and moves 8-byte vectors.
//    The 4 waves of a workgroup stack along the CHANNEL axis (N = 4K is the wide side: 416 pixels x 2048 channels at 1/32
//    scale and batch 8 are 13 x 16 workgroups) and share the pixel rows through the L1.
// 2. Junction backward, ONE streaming launch: g = g_out_next + g_pre [pre > 0] s (the gradient at `out`: feeds the data- and
//    weight-gradient GEMMs of _3_conv and IS the shortcut gradient; for a strided shortcut it is also scattered to the even
//    pixels of the input map, zeros elsewhere) and per-workgroup partial sums of db3 / dbeta / dgamma.  The ReLU mask is
//    recomputed from the stored 16-bit `out` with the forward's own expression (rj_affine): bit-identical masks.  Fixed
//    summation order, no atomics.
// 3. pool1: ZeroPadding2D(1) + MaxPooling2D(3, strides 2).  The padding is ZEROS that take part in the max (the conv1_conv
//    output is signed).  TIE RULE: the FIRST maximal tap in row-major window order wins (padded taps included: a winning
//    padded tap drops the gradient); the forward records the winning tap, the backward gathers by it.
#include "xpt_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef xpt_h16x8 h16x8;

struct RjBn {
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* var;
  float eps;
};

// scale / shift of the inference BatchNorm and the pre-activation value: ONE definition for forward and backward
__device__ __forceinline__ void rj_scale_shift(const RjBn& bn, int n, float& s, float& t) {
  s = bn.gamma[n] * rsqrtf(bn.var[n] + bn.eps);
  t = fmaf(-bn.mean[n], s, bn.beta[n]);
}
__device__ __forceinline__ float rj_affine(float out, float s, float t) { return fmaf(out, s, t); }

constexpr int RJ_G = 8;        // k steps (of 16) whose loads are issued together

// acc += W[rows of this wave][0..K) x X[pixels of this wave][0..K)^T; K % 8 == 0
__device__ __forceinline__ void rj_gemm(f32x16& acc, const unsigned short* __restrict__ wrow, bool w_ok,
                                        const unsigned short* __restrict__ xrow, int K, int h) {
  const int ksteps = (K + 15) >> 4;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  for (int s0 = 0; s0 < ksteps; s0 += RJ_G) {
    uint4 fa[RJ_G], fb[RJ_G];
#pragma unroll
    for (int g = 0; g < RJ_G; ++g) {                   // unconditional loads from a clamped k, zeroed by select
      const int k = (s0 + g) * 16 + 8 * h;
      const bool ok = k < K;
      const int kc = ok ? k : 0;
      const uint4 a = *(const uint4*)(wrow + kc), b = *(const uint4*)(xrow + kc);
      fa[g] = (ok && w_ok) ? a : zero;
      fb[g] = ok ? b : zero;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < RJ_G; ++g)
      if (s0 + g < ksteps)                             // wave-uniform
        acc = XPT_MFMA_32X32X16(__builtin_bit_cast(h16x8, fa[g]), __builtin_bit_cast(h16x8, fb[g]), acc);
  }
}

struct RjArgs {
  const unsigned short* h;      // [M, K] pixel pitch hpitch
  const unsigned short* w;      // [N, K]
  const float* bias;            // [N] or null
  const unsigned short* sx;     // conv shortcut: [M, SK] pixel pitch spitch, or null
  const unsigned short* sw;     // [N, SK]
  const float* sbias;           // [N] or null
  const unsigned short* sc;     // identity / strided shortcut: dense [rows of the input map, N], or null
  unsigned short* out;          // [M, N]
  unsigned short* pre;          // [M, N]
  RjBn bn;
  long long hpitch, spitch;
  int M, K, N, SK;
  int stride, OH, OW, IH, IW;   // stride 2: sc row of pixel (b, oy, ox) is (b IH + 2 oy) IW + 2 ox
};

__global__ __launch_bounds__(256) void res_join_fwd_kernel(RjArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * 32;
  const int n0 = (blockIdx.y * 4 + wave) * 32;
  if (n0 >= a.N || m0 >= a.M) return;                  // wave-uniform; the kernel has no barrier
  const int m = m0 + r;
  const bool pok = m < a.M;
  const int mm = pok ? m : a.M - 1;                    // rows past the end re-read the last row (never stored)
  const int nrow = n0 + r;
  const bool nok = nrow < a.N;
  const int nn = nok ? nrow : a.N - 1;

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  rj_gemm(acc, a.w + (long long)nn * a.K, nok, a.h + (long long)mm * a.hpitch, a.K, h);
  if (a.sx != nullptr) rj_gemm(acc, a.sw + (long long)nn * a.SK, nok, a.sx + (long long)mm * a.spitch, a.SK, h);

  long long srow = mm;
  if (a.sc != nullptr && a.stride == 2) {
    unsigned ox, oy;
    const unsigned q = xpt_divmod((unsigned)mm, (unsigned)a.OW, ox);
    const unsigned b = xpt_divmod(q, (unsigned)a.OH, oy);
    srow = ((long long)b * a.IH + 2 * (int)oy) * a.IW + 2 * (int)ox;
  }
  // register 4 qg + e: channel n0 + 8 qg + 4 h + e of pixel m
#pragma unroll
  for (int qg = 0; qg < 4; ++qg) {
    const int n = n0 + 8 * qg + 4 * h;
    if (!pok || n >= a.N) continue;                    // N % 8 == 0: a group of 4 channels is inside or outside as a whole
    uint2 sraw = make_uint2(0u, 0u);
    if (a.sc != nullptr) sraw = *(const uint2*)(a.sc + srow * a.N + n);
    const float sv[4] = {xpt_h2f_lo(sraw.x), xpt_h2f_hi(sraw.x), xpt_h2f_lo(sraw.y), xpt_h2f_hi(sraw.y)};
    unsigned short o[4], p[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = acc[4 * qg + e];
      if (a.bias != nullptr) v += a.bias[n + e];
      if (a.sbias != nullptr) v += a.sbias[n + e];
      v += sv[e];
      o[e] = xpt_f2h(v);
      float s, t;
      rj_scale_shift(a.bn, n + e, s, t);
      // the BatchNorm sees the ROUNDED junction output, as the backward (and a composed path) does
      p[e] = xpt_f2h(fmaxf(rj_affine(xpt_h2f(o[e]), s, t), 0.f));
    }
    const long long off = (long long)m * a.N + n;
    *(uint2*)(a.out + off) = make_uint2((unsigned)o[0] | ((unsigned)o[1] << 16), (unsigned)o[2] | ((unsigned)o[3] << 16));
    *(uint2*)(a.pre + off) = make_uint2((unsigned)p[0] | ((unsigned)p[1] << 16), (unsigned)p[2] | ((unsigned)p[3] << 16));
  }
}

// ------------------------------------------------------------------------------------------------ junction backward
struct RjBwdArgs {
  const unsigned short* g_out;  // dense [M, N] or null
  const unsigned short* g_pre;  // dense [M, N] or null
  const unsigned short* out;    // dense [M, N]
  unsigned short* g;            // dense [M, N]
  unsigned short* gs;           // strided shortcut: dense [B IH IW, N] (every pixel written), else null
  float* part;                  // [nblk][3][N]: db3, dbeta, dgamma
  RjBn bn;
  int M, N, rows_per_blk;
  int OH, OW, IH, IW;
};

constexpr int RJ_RED_PITCH = 25;   // 24 sums per thread, odd pitch

// rows of a workgroup / row slots per pass for a channel count (shared by host and device)
__host__ __device__ inline int rj_groups_local(int N, int by) {
  const int ng = N >> 3, left = ng - by * 256;
  return left < 256 ? left : 256;
}

__global__ __launch_bounds__(256) void res_join_bwd_kernel(RjBwdArgs a) {
  __shared__ float red[256 * RJ_RED_PITCH];
  const int tid = threadIdx.x;
  const int ngl = rj_groups_local(a.N, blockIdx.y);      // 8-channel groups of this workgroup (1 .. 256)
  const int rp = 256 / ngl;                              // row slots per pass
  const int cg = tid % ngl, rr = tid / ngl;
  const bool live = rr < rp;
  const int n = (blockIdx.y * 256 + cg) * 8;
  float s[8], t[8], mean[8], rstd[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    rj_scale_shift(a.bn, n + e, s[e], t[e]);
    mean[e] = a.bn.mean[n + e];
    rstd[e] = rsqrtf(a.bn.var[n + e] + a.bn.eps);
  }
  float sum_b3[8], sum_beta[8], sum_gamma[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sum_b3[e] = sum_beta[e] = sum_gamma[e] = 0.f;
  const int row_begin = blockIdx.x * a.rows_per_blk;
  const int row_end = row_begin + a.rows_per_blk < a.M ? row_begin + a.rows_per_blk : a.M;
  if (live) {
    for (int m = row_begin + rr; m < row_end; m += rp) {
      const long long off = (long long)m * a.N + n;
      const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
      const uint4 o4 = *(const uint4*)(a.out + off);
      const uint4 gp4 = a.g_pre != nullptr ? *(const uint4*)(a.g_pre + off) : zero;
      const uint4 go4 = a.g_out != nullptr ? *(const uint4*)(a.g_out + off) : zero;
      const unsigned* ow = (const unsigned*)&o4;
      const unsigned* gpw = (const unsigned*)&gp4;
      const unsigned* gow = (const unsigned*)&go4;
      uint4 g4;
      unsigned* gw = (unsigned*)&g4;
#pragma unroll
      for (int e2 = 0; e2 < 4; ++e2) {
        unsigned short pk[2];
#pragma unroll
        for (int hi = 0; hi < 2; ++hi) {
          const int e = 2 * e2 + hi;
          const float o = hi ? xpt_h2f_hi(ow[e2]) : xpt_h2f_lo(ow[e2]);
          const float gp = hi ? xpt_h2f_hi(gpw[e2]) : xpt_h2f_lo(gpw[e2]);
          const float go = hi ? xpt_h2f_hi(gow[e2]) : xpt_h2f_lo(gow[e2]);
          const float gm = rj_affine(o, s[e], t[e]) > 0.f ? gp : 0.f;     // the forward's own expression: the same mask
          const float gv = fmaf(gm, s[e], go);
          pk[hi] = xpt_f2h(gv);
          const float gr = xpt_h2f(pk[hi]);            // db3 sums what the GEMMs of _3_conv see
          sum_b3[e] += gr;
          sum_beta[e] += gm;
          sum_gamma[e] += gm * ((o - mean[e]) * rstd[e]);
        }
        gw[e2] = (unsigned)pk[0] | ((unsigned)pk[1] << 16);
      }
      *(uint4*)(a.g + off) = g4;
      if (a.gs != nullptr) {
        // MaxPooling2D(1, strides=2) backward: g lands on pixel (2 oy, 2 ox); the other pixels of that 2 x 2 cell get zeros
        // (every input pixel belongs to exactly one cell: no memset, no second launch)
        unsigned ox, oy;
        const unsigned q = xpt_divmod((unsigned)m, (unsigned)a.OW, ox);
        const unsigned b = xpt_divmod(q, (unsigned)a.OH, oy);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
          for (int dx = 0; dx < 2; ++dx) {
            const int iy = 2 * (int)oy + dy, ix = 2 * (int)ox + dx;
            if (iy < a.IH && ix < a.IW)
              *(uint4*)(a.gs + (((long long)b * a.IH + iy) * a.IW + ix) * a.N + n) = (dy | dx) ? zero : g4;
          }
      }
    }
  }
  float* mine = red + tid * RJ_RED_PITCH;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    mine[e] = sum_b3[e];
    mine[8 + e] = sum_beta[e];
    mine[16 + e] = sum_gamma[e];
  }
  __syncthreads();
  if (rr == 0) {                                         // row slots added in slot order
    float* dst = a.part + (long long)blockIdx.x * 3 * a.N;
#pragma unroll
    for (int j = 0; j < 24; ++j) {
      float acc = 0.f;
      for (int q = 0; q < rp; ++q) acc += red[(q * ngl + cg) * RJ_RED_PITCH + j];
      dst[(j >> 3) * a.N + n + (j & 7)] = acc;
    }
  }
}

int rj_rows_per_block(int M, int N) {
  const int ngl = rj_groups_local(N, 0);
  const int rp = 256 / ngl;
  int rows = (M + 255) / 256;                            // at most 256 partial rows (one GradSink pass)
  if (rows < 4 * rp) rows = 4 * rp;
  return (rows + rp - 1) / rp * rp;
}

// ------------------------------------------------------------------------------------------------ pool1
struct PoolArgs {
  const unsigned short* x;      // [B, H, W, C]
  unsigned short* y;            // [B, OH, OW, C]
  unsigned char* idx;           // [B, OH, OW, C]: winning tap 0..8 (row-major in the window)
  int B, H, W, C, OH, OW;
  unsigned total;               // threads: B OH OW C/8 (forward), B H W C/8 (backward)
};

__global__ __launch_bounds__(256) void maxpool3s2_zero_fwd_kernel(PoolArgs a) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.total) return;
  int cg, ox, oy, b;
  xpt_split4(i, a.C >> 3, a.OW, a.OH, cg, ox, oy, b);
  float best[8];
  unsigned char bi[8];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int iy = 2 * oy - 1 + tap / 3, ix = 2 * ox - 1 + tap % 3;
    const bool ok = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);              // the padding: 0.0, a candidate like any other
    if (ok) v = *(const uint4*)(a.x + (((long long)b * a.H + iy) * a.W + ix) * a.C + cg * 8);
    const unsigned* vw = (const unsigned*)&v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = (e & 1) ? xpt_h2f_hi(vw[e >> 1]) : xpt_h2f_lo(vw[e >> 1]);
      if (tap == 0 || f > best[e]) {                   // strict: the FIRST maximal tap wins
        best[e] = f;
        bi[e] = (unsigned char)tap;
      }
    }
  }
  uint4 yv;
  unsigned* yw = (unsigned*)&yv;
  uint2 iv;
  unsigned char* ib = (unsigned char*)&iv;
#pragma unroll
  for (int e = 0; e < 8; e += 2) yw[e >> 1] = (unsigned)xpt_f2h(best[e]) | ((unsigned)xpt_f2h(best[e + 1]) << 16);
#pragma unroll
  for (int e = 0; e < 8; ++e) ib[e] = bi[e];
  const long long o = (((long long)b * a.OH + oy) * a.OW + ox) * a.C + cg * 8;
  *(uint4*)(a.y + o) = yv;
  *(uint2*)(a.idx + o) = iv;
}

// dx[b, y, x, c] = sum over the (at most 2 x 2) windows that contain the pixel and whose winning tap it is; window order
__global__ __launch_bounds__(256) void maxpool3s2_zero_bwd_kernel(PoolArgs a, const unsigned short* __restrict__ dy,
                                                                  unsigned short* __restrict__ dx) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.total) return;
  int cg, x, y, b;
  xpt_split4(i, a.C >> 3, a.W, a.H, cg, x, y, b);
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  // windows oy with 2 oy - 1 <= y <= 2 oy + 1
  const int oy_lo = y >> 1, oy_hi = (y + 1) >> 1, ox_lo = x >> 1, ox_hi = (x + 1) >> 1;
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {
    if (oy >= a.OH) continue;
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      if (ox >= a.OW) continue;
      const int tap = (y - (2 * oy - 1)) * 3 + (x - (2 * ox - 1));
      const long long o = (((long long)b * a.OH + oy) * a.OW + ox) * a.C + cg * 8;
      const uint2 iv = *(const uint2*)(a.idx + o);
      const uint4 gv = *(const uint4*)(dy + o);
      const unsigned char* ib = (const unsigned char*)&iv;
      const unsigned* gw = (const unsigned*)&gv;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = (e & 1) ? xpt_h2f_hi(gw[e >> 1]) : xpt_h2f_lo(gw[e >> 1]);
        if ((int)ib[e] == tap) acc[e] += g;
      }
    }
  }
  uint4 out;
  unsigned* ow = (unsigned*)&out;
#pragma unroll
  for (int e = 0; e < 8; e += 2) ow[e >> 1] = (unsigned)xpt_f2h(acc[e]) | ((unsigned)xpt_f2h(acc[e + 1]) << 16);
  *(uint4*)(dx + (((long long)b * a.H + y) * a.W + x) * a.C + cg * 8) = out;
}

bool aligned16(const void* p) { return ((uintptr_t)p) % 16 == 0; }

}  // namespace

extern "C" int xpt_res_join_fwd(const void* h, long long hpitch, const void* w3, const float* b3, const void* sc_x,
                                long long sc_pitch, const void* sc_w, const float* sc_b, int sc_k, const void* shortcut,
                                const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                                void* out, void* pre, long long M, int K, int N, int stride, int OH, int OW, int IH, int IW,
                                void* stream) {
  XPT_CHECK_PTR(h); XPT_CHECK_PTR(w3); XPT_CHECK_PTR(gamma); XPT_CHECK_PTR(beta); XPT_CHECK_PTR(mean); XPT_CHECK_PTR(var);
  XPT_CHECK_PTR(out); XPT_CHECK_PTR(pre);
  if (M <= 0 || M >= 0x7fffffffLL || K <= 0 || N <= 0 || K % 8 != 0 || N % 8 != 0 || hpitch < K || hpitch % 8 != 0)
    return XPT_ERR_SHAPE;
  if (!aligned16(h) || !aligned16(w3) || !aligned16(out) || !aligned16(pre) || !aligned16(shortcut)) return XPT_ERR_ARG;
  if (sc_x != nullptr) {
    XPT_CHECK_PTR(sc_w);
    if (sc_k <= 0 || sc_k % 8 != 0 || sc_pitch < sc_k || sc_pitch % 8 != 0) return XPT_ERR_SHAPE;
    if (!aligned16(sc_x) || !aligned16(sc_w) || shortcut != nullptr) return XPT_ERR_ARG;
  }
  if (stride != 1 && stride != 2) return XPT_ERR_ARG;
  if (stride == 2) {
    if (shortcut == nullptr) return XPT_ERR_ARG;
    if (OH <= 0 || OW <= 0 || IH <= 0 || IW <= 0 || OH >= (1 << 24) || OW >= (1 << 24) || M % ((long long)OH * OW) != 0)
      return XPT_ERR_SHAPE;
    if (2 * (OH - 1) >= IH || 2 * (OW - 1) >= IW) return XPT_ERR_SHAPE;      // the last selected pixel lies inside the input map
  }
  const long long gy = (N + 127) / 128;
  if (gy > 65535) return XPT_ERR_SHAPE;
  RjArgs a{};
  a.h = (const unsigned short*)h; a.w = (const unsigned short*)w3; a.bias = b3;
  a.sx = (const unsigned short*)sc_x; a.sw = (const unsigned short*)sc_w; a.sbias = sc_x != nullptr ? sc_b : nullptr;
  a.sc = (const unsigned short*)shortcut;
  a.out = (unsigned short*)out; a.pre = (unsigned short*)pre;
  a.bn = RjBn{gamma, beta, mean, var, eps};
  a.hpitch = hpitch; a.spitch = sc_pitch;
  a.M = (int)M; a.K = K; a.N = N; a.SK = sc_k;
  a.stride = stride; a.OH = OH; a.OW = OW; a.IH = IH; a.IW = IW;
  const dim3 grid((unsigned)((M + 31) / 32), (unsigned)gy);
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(res_join_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return xpt_launch_status();
}

extern "C" int xpt_res_join_bwd_blocks(long long M, int N) {
  if (M <= 0 || M >= 0x7fffffffLL || N <= 0 || N % 8 != 0) return XPT_ERR_SHAPE;
  const int rows = rj_rows_per_block((int)M, N);
  return (int)((M + rows - 1) / rows);
}

extern "C" int xpt_res_join_bwd(const void* g_out_next, const void* g_pre, const void* out, const float* gamma,
                                const float* beta, const float* mean, const float* var, float eps, void* g,
                                void* g_shortcut, float* partials, size_t partial_floats, long long M, int N, int stride,
                                int OH, int OW, int IH, int IW, void* stream) {
  XPT_CHECK_PTR(out); XPT_CHECK_PTR(gamma); XPT_CHECK_PTR(beta); XPT_CHECK_PTR(mean); XPT_CHECK_PTR(var); XPT_CHECK_PTR(g);
  XPT_CHECK_PTR(partials);
  if (M <= 0 || M >= 0x7fffffffLL || N <= 0 || N % 8 != 0) return XPT_ERR_SHAPE;
  if (!aligned16(g_out_next) || !aligned16(g_pre) || !aligned16(out) || !aligned16(g) || !aligned16(g_shortcut))
    return XPT_ERR_ARG;
  if (stride != 1 && stride != 2) return XPT_ERR_ARG;
  if ((stride == 2) != (g_shortcut != nullptr)) return XPT_ERR_ARG;
  if (stride == 2) {
    if (OH <= 0 || OW <= 0 || IH <= 0 || IW <= 0 || OH >= (1 << 24) || OW >= (1 << 24) || M % ((long long)OH * OW) != 0)
      return XPT_ERR_SHAPE;
    if ((IH + 1) / 2 != OH || (IW + 1) / 2 != OW) return XPT_ERR_SHAPE;      // the 2 x 2 cells tile the input map exactly
  }
  const int rows = rj_rows_per_block((int)M, N);
  const int nblk = (int)((M + rows - 1) / rows);
  if (partial_floats < (size_t)nblk * 3 * N) return XPT_ERR_WORKSPACE;
  const long long gy = ((N >> 3) + 255) / 256;
  if (gy > 65535) return XPT_ERR_SHAPE;
  RjBwdArgs a{};
  a.g_out = (const unsigned short*)g_out_next; a.g_pre = (const unsigned short*)g_pre; a.out = (const unsigned short*)out;
  a.g = (unsigned short*)g; a.gs = (unsigned short*)g_shortcut; a.part = partials;
  a.bn = RjBn{gamma, beta, mean, var, eps};
  a.M = (int)M; a.N = N; a.rows_per_blk = rows;
  a.OH = OH; a.OW = OW; a.IH = IH; a.IW = IW;
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(res_join_bwd_kernel, dim3(nblk, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, a);
  return xpt_launch_status();
}

static int pool_args(PoolArgs& a, int B, int H, int W, int C, int OH, int OW, bool backward) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0) return XPT_ERR_SHAPE;
  if (OH != (H - 1) / 2 + 1 || OW != (W - 1) / 2 + 1) return XPT_ERR_SHAPE;          // (H + 2 - 3) / 2 + 1
  const long long total = (long long)B * (backward ? (long long)H * W : (long long)OH * OW) * (C >> 3);
  if (total >= 0x7fffffffLL || H >= (1 << 24) || W >= (1 << 24) || (C >> 3) >= (1 << 24)) return XPT_ERR_SHAPE;
  a.B = B; a.H = H; a.W = W; a.C = C; a.OH = OH; a.OW = OW; a.total = (unsigned)total;
  return XPT_OK;
}

extern "C" int xpt_maxpool3s2_zero_fwd(const void* x, void* y, void* idx, int B, int H, int W, int C, int OH, int OW,
                                       void* stream) {
  XPT_CHECK_PTR(x); XPT_CHECK_PTR(y); XPT_CHECK_PTR(idx);
  if (!aligned16(x) || !aligned16(y) || !aligned16(idx)) return XPT_ERR_ARG;
  PoolArgs a{};
  const int rc = pool_args(a, B, H, W, C, OH, OW, false);
  if (rc != XPT_OK) return rc;
  a.x = (const unsigned short*)x; a.y = (unsigned short*)y; a.idx = (unsigned char*)idx;
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(maxpool3s2_zero_fwd_kernel, dim3((a.total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a);
  return xpt_launch_status();
}

extern "C" int xpt_maxpool3s2_zero_bwd(const void* dy, const void* idx, void* dx, int B, int H, int W, int C, int OH, int OW,
                                       void* stream) {
  XPT_CHECK_PTR(dy); XPT_CHECK_PTR(idx); XPT_CHECK_PTR(dx);
  if (!aligned16(dy) || !aligned16(idx) || !aligned16(dx)) return XPT_ERR_ARG;
  PoolArgs a{};
  const int rc = pool_args(a, B, H, W, C, OH, OW, true);
  if (rc != XPT_OK) return rc;
  a.idx = (unsigned char*)const_cast<void*>(idx);
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(maxpool3s2_zero_bwd_kernel, dim3((a.total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a,
                     (const unsigned short*)dy, (unsigned short*)dx);
  return xpt_launch_status();
}
