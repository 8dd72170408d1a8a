// clip_loss.hip -- stage-2 MambaXray-CLIP contrastive step as ONE kernel: L2-normalise image / text features, cosine
// logits * exp(logit_scale), symmetric cross-entropy, and every gradient of it.
//
// Replaces the eager sequence of CXPMRG_Bench_MambaXray_VL/models/MambaXrayVL_CLIP.py:133-148
//   image_features /= norm; text_features /= norm; logits = scale * img @ txt.t(); loss = (CE(logits) + CE(logits.t())) / 2
// (~25 small kernels forward + backward at batch 48 x 512: launch-bound).  The problem is tiny (2 x 98 KB of features, a
// 48 x 48 logit matrix): one workgroup keeps the logits and their gradient in LDS; features are read through L1/L2.
// Outputs the loss and, for d(loss) = 1, d(image_features), d(text_features), d(logit_scale); the autograd wrapper scales
// them by the incoming gradient.  fp32 features (the projections' outputs are cast up, as the reference's .float() loss).
// Beyond 89 rows (a global batch gathered over data-parallel ranks) the two n x n matrices no longer fit: 90 .. 4096 rows run as
// five launches that recompute the logits tile by tile on the f32 MFMA (second half of this file).
#include "mxvl_common.h"

namespace mxvl {

struct ClipArgs {
  int n, dim;
  const float* logit_scale;   // device scalar: the PARAMETER (log of the multiplier)
  const float *img, *txt;
  float *loss, *dimg, *dtxt, *dscale;
};

__device__ inline float wave_sum64(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(1024) void clip_loss_kernel(const ClipArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int n = p.n, P = p.dim, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NW = 16;
  float* sL = sm;                 // [n][n] logits
  float* sG = sL + n * n;         // [n][n] d loss / d logits
  float* inv_i = sG + n * n;      // [n] 1 / |img_i|
  float* inv_t = inv_i + n;       // [n]
  float* lse_r = inv_t + n;       // [n] row log-sum-exp (image -> text)
  float* lse_c = lse_r + n;       // [n] column log-sum-exp (text -> image)
  float* red = lse_c + n;         // [NW] scratch
  const float s = __expf(*p.logit_scale);

  for (int r = wave; r < 2 * n; r += NW) {            // row norms: one wave per row
    const float* x = (r < n ? p.img + (size_t)r * P : p.txt + (size_t)(r - n) * P);
    float a = 0.f;
    for (int k = lane; k < P; k += 64) a = fmaf(x[k], x[k], a);
    a = wave_sum64(a);
    if (lane == 0) (r < n ? inv_i[r] : inv_t[r - n]) = rsqrtf(a);
  }
  __syncthreads();
  for (int e = wave; e < n * n; e += NW) {             // logits: one wave per (i, j)
    const int i = e / n, j = e - i * n;
    const float *x = p.img + (size_t)i * P, *y = p.txt + (size_t)j * P;
    float a = 0.f;
    for (int k = lane; k < P; k += 64) a = fmaf(x[k], y[k], a);
    a = wave_sum64(a);
    if (lane == 0) sL[e] = s * a * inv_i[i] * inv_t[j];
  }
  __syncthreads();
  if (tid < 2 * n) {                                   // log-sum-exp of every row and every column
    const int r = tid < n ? tid : tid - n;
    float mx = -__builtin_inff();
    for (int k = 0; k < n; ++k) mx = fmaxf(mx, tid < n ? sL[r * n + k] : sL[k * n + r]);
    float a = 0.f;
    for (int k = 0; k < n; ++k) a += __expf((tid < n ? sL[r * n + k] : sL[k * n + r]) - mx);
    (tid < n ? lse_r : lse_c)[r] = mx + __logf(a);
  }
  __syncthreads();
  float part = 0.f, dsc = 0.f;                          // loss and d/d(logit_scale)
  const float w = 0.5f / (float)n;
  for (int e = tid; e < n * n; e += 1024) {
    const int i = e / n, j = e - i * n;
    const float l = sL[e];
    const float g = w * (__expf(l - lse_r[i]) + __expf(l - lse_c[j]) - (i == j ? 2.f : 0.f));
    sG[e] = g;
    dsc = fmaf(g, l, dsc);                              // d logits / d logit_scale = logits  (multiplier = exp(param))
    if (i == j) part += w * ((lse_r[i] - l) + (lse_c[i] - l));
  }
  part = wave_sum64(part);
  dsc = wave_sum64(dsc);
  if (lane == 0) { red[wave] = part; red[NW + wave] = dsc; }
  __syncthreads();
  if (tid == 0) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < NW; ++k) { a += red[k]; b += red[NW + k]; }
    *p.loss = a;
    *p.dscale = b;
  }
  // d normalised features, then back through x / |x|:  dx = (dn - n (n . dn)) / |x|
  for (int r = wave; r < 2 * n; r += NW) {
    const bool is_img = r < n;
    const int i = is_img ? r : r - n;
    const float* x = (is_img ? p.img : p.txt) + (size_t)i * P;
    float* dx = (is_img ? p.dimg : p.dtxt) + (size_t)i * P;
    const float ix = is_img ? inv_i[i] : inv_t[i];
    float dot = 0.f;
    for (int k = lane; k < P; k += 64) {
      float a = 0.f;
      for (int j = 0; j < n; ++j) {
        const float g = is_img ? sG[i * n + j] : sG[j * n + i];
        const float y = (is_img ? p.txt : p.img)[(size_t)j * P + k] * (is_img ? inv_t[j] : inv_i[j]);
        a = fmaf(g, y, a);
      }
      a *= s;
      dx[k] = a;                     // d n_k, finished below
      dot = fmaf(a, x[k] * ix, dot);
    }
    dot = wave_sum64(dot);
    for (int k = lane; k < P; k += 64) dx[k] = (dx[k] - x[k] * ix * dot) * ix;   // same lane wrote dx[k]: no hazard
  }
}

// ---- 90 <= batch <= 4096: five launches on the caller's stream -------------------------------------------------------------------
// The n x n logits no longer fit one workgroup's LDS, so they are never stored: every launch recomputes the 32 x 32 tiles it needs
// on the exact-f32 matrix path (v_mfma_f32_32x32x2_f32 == an fmaf chain, bit for bit).  What has to survive a kernel boundary is
// 8n floats, and since the entry has no workspace parameter they live in the first 8n floats of d_image until the last launch
// overwrites them with gradient rows:
//   [0, n) 1/|img_i|   [n, 2n) 1/|txt_j|   [2n, 3n) row max m_r   [3n, 4n) log sum exp(l - m_r)   [4n, 5n) column max m_c
//   [5n, 6n) log sum exp(l - m_c)   [6n, 7n) loss term of index i   [7n, 8n) sum_i g_ij l_ij of column j
// (max and log-sum kept apart: exp((l - m) - log_sum) loses nothing to the magnitude of m when logit_scale is at its clamp of 100).
//   1 clip_norms_kernel   -> [0, 2n)
//   2 clip_lse_kernel     grid (tiles, 2): a tile of image rows x all text rows, and with the operands swapped a tile of text rows x
//                         all image rows; online log-sum-exp per lane, merged in lane / wave order -> [2n, 6n)
//   3 clip_grad_kernel<1> a tile of text rows x all image rows: g, d txt_n = s sum_i g_ij img_n_i, back through the normalisation
//                         -> final d_text; the loss term and sum_i g_ij l_ij of its columns -> [6n, 8n)
//   4 clip_grad_kernel<0> the same body for the image rows from R0 = ceil(8n / dim) on: reads the scratch (rows below R0), writes
//                         only rows >= R0
//   5 clip_head_kernel    ONE workgroup: copies the 8n floats to LDS, barrier, folds loss and d_logit_scale in a fixed tree, then runs
//                         the gradient body for image rows [0, R0) with the scratch read from LDS.
// <x_n, d x_n> of the normalisation's backward is sum_j g_ij l_ij (l_ij = s <img_n_i, txt_n_j>), so it needs no reduction over dim.
// No atomics, no workgroup waits for another, every cross-lane / cross-wave / cross-workgroup sum has one fixed order: the same
// bits on every run and in both settings of mxvl_set_deterministic.
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kClipThreads = 256;      // 4 waves
constexpr int kClipGs = 33;            // row stride of a g tile in LDS: column reads hit distinct banks
constexpr int kClipChunk = 512;        // output columns of one gradient workgroup: 4 waves x 4 accumulator tiles x 32
constexpr int kClipMaxBatch = 4096;

struct ClipBigArgs {
  int n, dim, vec;            // vec: dim % 4 == 0 and 16-byte aligned feature pointers
  const float* logit_scale;
  const float *img, *txt;
  float *loss, *dimg, *dtxt, *dscale;
};
struct ClipSh {
  float gs[4][32 * kClipGs];  // one g tile (own row, other row) per wave, scaled by 1 / |other|
  float red[4][32];
  float lterm[32];
};

__device__ inline int clip_crow(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }   // C/D row of a 32x32 MFMA
// one expression for l_ij wherever it is recomputed: the launches agree bit for bit
// exp(logit_scale) multiplies EVERY logit, so its rounding is the one error that does not average out over the batch (at the clamp
// of 100 half an ulp of it moves the loss by d_logit_scale * 6e-8): it is carried as hi + lo of its float64 value.
struct ClipScale { float hi, lo; };
__device__ inline ClipScale clip_scale(const float* logit_scale) {
  const double sd = exp((double)*logit_scale);
  ClipScale s;
  s.hi = (float)sd;
  s.lo = (float)(sd - (double)s.hi);
  return s;
}
__device__ inline float clip_logit(float dot, float inv_img, float inv_txt, ClipScale s) {
  const float c = (dot * inv_img) * inv_txt;
  return fmaf(s.hi, c, s.lo * c);
}

__device__ inline float4 clip_ld4(const float* row, int c, int P, bool vec) {
  if (vec) return c < P ? *(const float4*)(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  return make_float4(c < P ? row[c] : 0.f, c + 1 < P ? row[c + 1] : 0.f, c + 2 < P ? row[c + 2] : 0.f, c + 3 < P ? row[c + 3] : 0.f);
}

// <a_row of lane & 31, b_row of lane & 31> for the 32 x 32 pairs of a wave.  The MFMA's k index is only a summation index: lane half h
// feeds columns 8 t + 4 h .. + 3 of both operands (one 16-byte load each), so MFMA e of step t pairs columns 8t + e and 8t + 4 + e.
__device__ inline f32x16 clip_tile_dots(const float* a_row, const float* b_row, int P, bool vec, int h) {
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int P8 = (P + 7) & ~7;
#pragma unroll 4
  for (int c = 4 * h; c < P8; c += 8) {
    const float4 a = clip_ld4(a_row, c, P, vec), b = clip_ld4(b_row, c, P, vec);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  }
  return acc;
}

__global__ __launch_bounds__(kClipThreads) void clip_norms_kernel(const ClipBigArgs p) {
  const int n = p.n, P = p.dim, lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= 2 * n) return;
  const float* x = (r < n ? p.img + (size_t)r * P : p.txt + (size_t)(r - n) * P);
  float a = 0.f;
  for (int k = lane; k < P; k += 64) a = fmaf(x[k], x[k], a);
  a = wave_sum64(a);
  if (lane == 0) p.dimg[r] = 1.0f / sqrtf(a);
}

// (m, a) <- (m, a) (+) (m2, a2):  sum exp(l) = a exp(m)
__device__ inline void clip_lse_merge(float& m, float& a, float m2, float a2) {
  const float mn = fmaxf(m, m2);
  const float e1 = m == mn ? 1.f : expf(m - mn), e2 = m2 == mn ? 1.f : expf(m2 - mn);   // (-inf, 0) (+) (-inf, 0) stays (-inf, 0)
  a = a * e1 + a2 * e2;
  m = mn;
}

// blockIdx.y = side: 0 image rows against all text rows (row log-sum-exp), 1 text rows against all image rows (column log-sum-exp)
__global__ __launch_bounds__(kClipThreads) void clip_lse_kernel(const ClipBigArgs p) {
  __shared__ float sm[4][32], sa[4][32];
  const int n = p.n, P = p.dim, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c31 = lane & 31;
  const int side = blockIdx.y, own0 = blockIdx.x * 32, NT = (n + 31) / 32;
  const float *own = side ? p.txt : p.img, *oth = side ? p.img : p.txt;
  float* S = p.dimg;
  const float *inv_own = S + (size_t)side * n, *inv_oth = S + (size_t)(1 - side) * n;
  const ClipScale s = clip_scale(p.logit_scale);
  const float* a_row = own + (size_t)min(own0 + c31, n - 1) * P;
  float io[16], m[16], a[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    io[r] = inv_own[min(own0 + clip_crow(r, lane), n - 1)];
    m[r] = -__builtin_inff();
    a[r] = 0.f;
  }
  for (int ot = wave; ot < NT; ot += 4) {
    const int col = ot * 32 + c31, colc = min(col, n - 1);
    const f32x16 d = clip_tile_dots(a_row, oth + (size_t)colc * P, P, p.vec, h);
    const float ix = inv_oth[colc];
    if (col < n) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float l = clip_logit(d[r], side ? ix : io[r], side ? io[r] : ix, s);
        const float mn = fmaxf(m[r], l);
        a[r] = a[r] * expf(m[r] - mn) + expf(l - mn);
        m[r] = mn;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {                     // the 32 lanes of a half hold the same rows: fold them, then the 4 waves, in a fixed order
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
      const float m2 = __shfl_xor(m[r], off, 64), a2 = __shfl_xor(a[r], off, 64);
      clip_lse_merge(m[r], a[r], m2, a2);
    }
    if (c31 == 0) { sm[wave][clip_crow(r, lane)] = m[r]; sa[wave][clip_crow(r, lane)] = a[r]; }
  }
  __syncthreads();
  if (tid < 32 && own0 + tid < n) {
    float mm = sm[0][tid], aa = sa[0][tid];
    for (int w = 1; w < 4; ++w) clip_lse_merge(mm, aa, sm[w][tid], sa[w][tid]);
    float* dst = S + (size_t)2 * n + (size_t)side * 2 * n;
    dst[own0 + tid] = mm;
    dst[n + own0 + tid] = (float)log((double)aa);   // once per row: every loss term carries it, so a one-sided ulp of v_log_f32 would not average out
  }
}

// The gradient rows [row_lo, row_hi) of the 32 own rows from own0, output columns [pc * 512, pc * 512 + 512); side 0 = image rows,
// 1 = text rows.  S is the scratch: d_image itself, or the last launch's copy of it in LDS.  keep: store the loss terms and
// sum g l of the own rows to Sg[6n, 8n).  Every thread of the workgroup calls it.  g here is 2n times the issue's g_ij: the weight
// 1 / (2n) is applied once per output (a true division for the two scalars), not rounded into every element of every sum.
__device__ inline void clip_grad_tile(const ClipBigArgs& p, const float* S, int side, int own0, int pc, int row_lo, int row_hi, bool keep,
                                      float* Sg, ClipSh& sh, ClipScale s) {
  const int n = p.n, P = p.dim, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c31 = lane & 31;
  const int NT = (n + 31) / 32;
  const float *own = side ? p.txt : p.img, *oth = side ? p.img : p.txt;
  float* out = side ? p.dtxt : p.dimg;
  const float *inv_own = S + (size_t)side * n, *inv_oth = S + (size_t)(1 - side) * n;
  const float *mx_own = S + (size_t)2 * n + (size_t)side * 2 * n, *la_own = mx_own + n;
  const float *mx_oth = S + (size_t)2 * n + (size_t)(1 - side) * 2 * n, *la_oth = mx_oth + n;
  const float w = 0.5f / (float)n, sw = (float)(((double)s.hi + (double)s.lo) * 0.5 / (double)n);
  const float* a_row = own + (size_t)min(own0 + c31, n - 1) * P;
  float io[16], mo[16], lo[16], dsum[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int g = min(own0 + clip_crow(r, lane), n - 1);
    io[r] = inv_own[g]; mo[r] = mx_own[g]; lo[r] = la_own[g];
    dsum[r] = 0.f;
  }
  f32x16 acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
  __syncthreads();                                     // the LDS of a previous tile is free
  for (int r0 = 0; r0 < NT; r0 += 4) {
    const int ot = r0 + wave;
    if (ot < NT) {                                      // this wave's g tile of the round: own rows x other rows of tile ot
      const int col = ot * 32 + c31, colc = min(col, n - 1);
      const f32x16 d = clip_tile_dots(a_row, oth + (size_t)colc * P, P, p.vec, h);
      const float ix = inv_oth[colc], mxo = mx_oth[colc], lao = la_oth[colc];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = clip_crow(r, lane), row = own0 + rl;
        const float l = clip_logit(d[r], side ? ix : io[r], side ? io[r] : ix, s);
        float g = expf((l - mo[r]) - lo[r]) + expf((l - mxo) - lao) - (row == col ? 2.f : 0.f);
        if (col >= n || row >= n) g = 0.f;
        dsum[r] = fmaf(g, l, dsum[r]);
        if (row == col && col < n) sh.lterm[rl] = (lo[r] + (mo[r] - l)) + (lao + (mxo - l));
        sh.gs[wave][rl * kClipGs + c31] = g * ix;
      }
    }
    __syncthreads();
    const int nt = min(4, NT - r0);
    for (int t = 0; t < nt; ++t) {                      // d own_n[rows, cols of this wave] += g tile t x other rows of tile r0 + t
#pragma unroll 4
      for (int ks = 0; ks < 16; ++ks) {
        const float a = sh.gs[t][c31 * kClipGs + 2 * ks + h];
        const float* b_row = oth + (size_t)min((r0 + t) * 32 + 2 * ks + h, n - 1) * P;   // rows past n meet g = 0
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const int c0 = pc * kClipChunk + (ct * 4 + wave) * 32;
          if (c0 < P) {
            const float b = c0 + c31 < P ? b_row[c0 + c31] : 0.f;
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[ct], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {                       // sum_other g l of the own rows: lanes, then waves, in a fixed order
    float v = dsum[r];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (c31 == 0) sh.red[wave][clip_crow(r, lane)] = v;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rl = clip_crow(r, lane), row = own0 + rl;
    const float dot = w * (((sh.red[0][rl] + sh.red[1][rl]) + sh.red[2][rl]) + sh.red[3][rl]);     // <own_n, d own_n>
    if (row >= row_lo && row < row_hi && row < n) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int pcol = pc * kClipChunk + (ct * 4 + wave) * 32 + c31;
        if (pcol < P) {
          const float xh = own[(size_t)row * P + pcol] * io[r];
          out[(size_t)row * P + pcol] = (sw * acc[ct][r] - xh * dot) * io[r];     // dx = (dn - n (n . dn)) / |x|
        }
      }
    }
  }
  if (keep && tid < 32 && own0 + tid < n) {
    Sg[(size_t)6 * n + own0 + tid] = sh.lterm[tid];
    Sg[(size_t)7 * n + own0 + tid] = ((sh.red[0][tid] + sh.red[1][tid]) + sh.red[2][tid]) + sh.red[3][tid];
  }
}

// SIDE 1: grid (text tiles, column chunks), final d_text and scratch [6n, 8n).  SIDE 0: grid (image tiles from R0 / 32 on, column
// chunks), d_image rows >= R0 = ceil(8n / dim) only: the scratch below stays readable for every workgroup of the launch.
template <int SIDE>
__global__ __launch_bounds__(kClipThreads) void clip_grad_kernel(const ClipBigArgs p) {
  __shared__ ClipSh sh;
  const int R0 = SIDE ? 0 : (8 * p.n + p.dim - 1) / p.dim;
  const int own0 = (R0 / 32 + (int)blockIdx.x) * 32;
  clip_grad_tile(p, p.dimg, SIDE, own0, blockIdx.y, R0, p.n, SIDE == 1 && blockIdx.y == 0, p.dimg, sh, clip_scale(p.logit_scale));
}

__global__ __launch_bounds__(kClipThreads) void clip_head_kernel(const ClipBigArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sS[];   // the 8n scratch floats
  __shared__ ClipSh sh;
  __shared__ double fold[2][kClipThreads];
  const int n = p.n, P = p.dim, tid = threadIdx.x;
  for (int e = tid; e < 8 * n; e += kClipThreads) sS[e] = p.dimg[e];
  __syncthreads();
  double a = 0.0, b = 0.0;   // 2n loss = sum of the loss terms, 2n d_logit_scale = sum of the column sums of g l: a fixed tree, in float64
  for (int j = tid; j < n; j += kClipThreads) { a += (double)sS[6 * n + j]; b += (double)sS[7 * n + j]; }
  fold[0][tid] = a; fold[1][tid] = b;
  __syncthreads();
  for (int st = kClipThreads / 2; st > 0; st >>= 1) {
    if (tid < st) { fold[0][tid] += fold[0][tid + st]; fold[1][tid] += fold[1][tid + st]; }
    __syncthreads();
  }
  if (tid == 0) { *p.loss = (float)(fold[0][0] / (2.0 * n)); *p.dscale = (float)(fold[1][0] / (2.0 * n)); }
  const int R0 = (8 * n + P - 1) / P;
  const ClipScale s = clip_scale(p.logit_scale);
  for (int own0 = 0; own0 < R0; own0 += 32)
    for (int pc = 0; pc * kClipChunk < P; ++pc) clip_grad_tile(p, sS, 0, own0, pc, 0, R0, false, nullptr, sh, s);
}

static int clip_loss_big(const ClipBigArgs& a, hipStream_t s) {
  const int n = a.n, P = a.dim, NT = (n + 31) / 32, NC = (P + kClipChunk - 1) / kClipChunk, R0 = (8 * n + P - 1) / P;
  const size_t lds = sizeof(float) * 8 * (size_t)n;    // + 21.6 KB static: 149 KB at 4096 rows
  if (lds > 40 * 1024 && hip_status(hipFuncSetAttribute((const void*)clip_head_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != MXVL_OK)
    return MXVL_ERR_LAUNCH;   // per call: the attribute belongs to the (kernel, device) pair
  hipLaunchKernelGGL(clip_norms_kernel, dim3((2 * n + 3) / 4), dim3(kClipThreads), 0, s, a);
  int st = launch_status();
  if (st != MXVL_OK) return st;
  hipLaunchKernelGGL(clip_lse_kernel, dim3(NT, 2), dim3(kClipThreads), 0, s, a);
  if ((st = launch_status()) != MXVL_OK) return st;
  hipLaunchKernelGGL(clip_grad_kernel<1>, dim3(NT, NC), dim3(kClipThreads), 0, s, a);
  if ((st = launch_status()) != MXVL_OK) return st;
  hipLaunchKernelGGL(clip_grad_kernel<0>, dim3(NT - R0 / 32, NC), dim3(kClipThreads), 0, s, a);
  if ((st = launch_status()) != MXVL_OK) return st;
  hipLaunchKernelGGL(clip_head_kernel, dim3(1), dim3(kClipThreads), lds, s, a);
  return launch_status();
}

}  // namespace mxvl

using namespace mxvl;

// batch <= 89: the single-workgroup kernel.  90 <= batch <= 4096 with dim >= 16: the five launches above (8 batch <= batch * dim / 2 scratch
// floats must fit below the d_image rows the fourth launch writes).  d_image and d_text hold intermediate values until the LAST
// launch of the call has finished.  Nothing is allocated, no device state is kept between calls.
extern "C" int mxvl_clip_loss(const float* image_features, const float* text_features, const float* logit_scale, int batch, int dim,
                              float* loss, float* d_image, float* d_text, float* d_logit_scale, void* hip_stream) {
  if (!image_features || !text_features || !logit_scale || !loss || !d_image || !d_text || !d_logit_scale) return MXVL_ERR_NULL;
  if (batch <= 0 || dim <= 0) return MXVL_ERR_SHAPE;
  const size_t lds = sizeof(float) * ((size_t)2 * batch * batch + 4 * batch + 32);
  if (lds > 64 * 1024) {                                 // batch > 89 (the reference trains stage 2 at batch 48 per GPU)
    if (batch > kClipMaxBatch || dim < 16) return MXVL_ERR_UNSUPPORTED;
    const int vec = dim % 4 == 0 && ((uintptr_t)image_features | (uintptr_t)text_features) % 16 == 0;
    ClipBigArgs b{batch, dim, vec, logit_scale, image_features, text_features, loss, d_image, d_text, d_logit_scale};
    return clip_loss_big(b, (hipStream_t)hip_stream);
  }
  ClipArgs a{batch, dim, logit_scale, image_features, text_features, loss, d_image, d_text, d_logit_scale};
  hipLaunchKernelGGL(clip_loss_kernel, dim3(1), dim3(1024), lds, (hipStream_t)hip_stream, a);
  return launch_status();
}
