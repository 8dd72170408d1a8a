// sample_step.hip -- one sampling update of the report decoder (HF `_sample` with do_sample=True) as ONE kernel, for gfx950.
//
// Replaces what HF `generate` runs per token between two decoder steps when the reference passes do_sample=True
// (EMRRG/models/MambaXrayVL_DownStream.py:440-449, 537-546; R2GenKG/models/R2GenKG.py:392-401, 480-489): RepetitionPenalty ->
// MinNewTokens -> Temperature -> TopK -> TopP -> softmax -> multinomial -- a full sort and a cumulative sum over rows x vocabulary and
// a dozen launches, the last of them not capturable.  Same rule, same order as report_decoder._SampleState.advance_torch, which is
// checked token-exact against HF; this kernel is tested against that function (include/mxvl.h states the contract and the tie rule).
//
// One workgroup (1024 threads) per row; the rows meet in ONE returning atomicAdd on the arrival word (as beam_step.hip does).
// Per row, every pass is a sweep of the row with 8 independent 16-byte loads in flight per lane:
//   A   logits -> processed scores in the workspace (temperature; then the <= max_new penalised history entries, the <= max_new
//       followers the no-repeat-n-gram rule bans (-inf, after the penalty: a ban wins) and the EOS ids are patched in place: the
//       patches are idempotent, so duplicates in the history write the same value)
//   1   row max + the first radix level of the top-k selection
//   2,3 the other two levels: the k-th largest score EXACTLY (the smallest key t with count{key > t} < k), no sort
//   4-6 the same three-level descent with a MASS per bucket instead of a count: the smallest key t with mass{key > t} < top_p * Z
//   F   kept mass of 16 contiguous parts of the row (one per wave), then the wave that holds u * Z walks its part in index order
// Passes 2-6 only run when their filter is on.  After pass A the row is read from L2 (a Qwen1.5 row is 600 KB).
// Determinism: counts and masses are 64-bit integers (mass = exp(score - max) in units of 2^-qbits, truncated), LDS histograms by
// integer atomics, so every sum is independent of the order it was formed in; no fp32 atomics anywhere.
#include <math.h>

#include "mxvl_common.h"

namespace mxvl {

constexpr int kSampThreads = 1024, kSampWaves = kSampThreads / kWave, kSampMaxEos = 4, kSampMaxRows = 80;
constexpr int kBins = 2048;                      // radix digits: 11 + 11 + 10 bits of the 32-bit key
typedef unsigned long long u64;

struct SampleArgs {
  int rows, V, max_new, min_new, n_eos, top_k, vec4, ngram;
  float rep_pen, temperature, top_p, mass_scale;  // mass_scale = 2^qbits
  long long fill;
  const float* logits;
  float* score;                                   // workspace: (rows, V) processed scores
  long long* seq; unsigned char* alive; long long* tok; long long* cur;
  const long long* eos; const long long* seed;
  unsigned char* unfinished; unsigned char* unf_log;
  unsigned int* ticket;
  float* out_thresh; int* out_kept;
};

// counter-based uniform: the mixer of attn.hip's attn_drop_hash over (low seed word, row, step, high seed word); a pure function,
// restated on the host by report_decoder.sample_uniform
__device__ __forceinline__ uint32_t sample_hash(u64 seed, uint32_t row, uint32_t step) {
  uint32_t x = (uint32_t)seed ^ (row * 0x9E3779B1u);
  x = (x ^ (step * 0x85EBCA77u)) * 0xC2B2AE3Du;
  x ^= (uint32_t)(seed >> 32) * 0x27D4EB2Fu;
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;     // murmur3's finaliser
  return x;
}

// order-preserving image of an fp32 score: a < b  <=>  key(a) < key(b)  (the scores are stored with -0 folded into +0)
__device__ __forceinline__ uint32_t score_key(float s) {
  const uint32_t b = __builtin_bit_cast(uint32_t, s);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// f(index, value) over row[0, V): float4 loads, 8 in flight per lane (scalar loads when the row is not 16-byte aligned)
template <typename F>
__device__ __forceinline__ void sweep(const float* __restrict__ row, int V, int vec4, F f) {
  const int tid = threadIdx.x;
  if (vec4) {
    const int n4 = V >> 2;
    const float4* r4 = (const float4*)row;
    for (int base = tid; base < n4; base += kSampThreads * 8) {
      float4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = base + j * kSampThreads;
        if (i < n4) v[j] = r4[i];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = base + j * kSampThreads;
        if (i < n4) { f(4 * i, v[j].x); f(4 * i + 1, v[j].y); f(4 * i + 2, v[j].z); f(4 * i + 3, v[j].w); }
      }
    }
  } else {
    for (int i = tid; i < V; i += kSampThreads) f(i, row[i]);
  }
}

__device__ __forceinline__ u64 wave_incl_scan(u64 v) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const u64 o = __shfl_up(v, d, kWave);
    if (lane >= d) v += o;
  }
  return v;
}

// The LDS the radix selection works in: a histogram of one digit and what descend leaves behind.
struct RadixLds { u64* hist; u64* wtot; u64* above; u64* incl; int* digit; };

// Thread t owns the digits hi = kBins - 1 - 2t and hi - 1 of L.hist (complete, barrier passed): thread order = descending digit
// order.  Returns the wave's inclusive scan of a + b and leaves every wave's total in L.wtot (a barrier passed).
__device__ __forceinline__ u64 hist_scan(const RadixLds& L, int hi, u64& a, u64& b) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  a = L.hist[hi]; b = L.hist[hi - 1];
  const u64 inc = wave_incl_scan(a + b);
  if (lane == kWave - 1) L.wtot[wave] = inc;
  __syncthreads();
  return inc;
}

// sum(L.hist); ends with the barrier that lets L.wtot be written again
__device__ __forceinline__ u64 hist_total(const RadixLds& L) {
  u64 a, b, z = 0;
  hist_scan(L, kBins - 1 - 2 * (int)threadIdx.x, a, b);
  for (int w = 0; w < kSampWaves; ++w) z += L.wtot[w];
  __syncthreads();
  return z;
}

// One level of the descent over L.hist (complete, barrier passed): the smallest digit d with above + sum(hist[> d]) < limit.
// Leaves d in *L.digit, above + sum(hist[> d]) in *L.above and above + sum(hist[>= d]) in *L.incl (read after the barrier it ends
// with).  sum(hist) + above >= limit is NOT required: when every digit passes, d = 0.
__device__ __forceinline__ void descend(const RadixLds& L, u64 above, u64 limit) {
  const int wave = threadIdx.x / kWave, hi = kBins - 1 - 2 * (int)threadIdx.x;
  u64 a, b;
  const u64 inc = hist_scan(L, hi, a, b);
  u64 before = above;
  for (int w = 0; w < wave; ++w) before += L.wtot[w];
  const u64 gt_hi = before + inc - (a + b);       // above + mass of the digits > hi
  const u64 gt_lo = gt_hi + a;                    // ... > hi - 1
  const u64 ge_lo = gt_lo + b;
  // digit d is the answer iff (above + M_>(d) < limit) and (d == 0 or above + M_>=(d) >= limit): exactly one digit qualifies
  if (gt_hi < limit && gt_lo >= limit) { *L.digit = hi; *L.above = gt_hi; *L.incl = gt_lo; }
  if (gt_lo < limit && (ge_lo >= limit || hi - 1 == 0)) { *L.digit = hi - 1; *L.above = gt_lo; *L.incl = ge_lo; }
  __syncthreads();
}

// Histogram of radix digit `level` (0 / 1 / 2: 11 + 11 + 10 bits of the key, top down) over the scores whose higher digits equal
// `prefix`'s: L.hist[digit] = sum of weight(score, key).  Zeroes first; ends with the barrier that completes the histogram.
template <typename W>
__device__ __forceinline__ void radix_fill(const RadixLds& L, const float* sc, int V, int vec4, int level, uint32_t prefix, W weight) {
  for (int i = threadIdx.x; i < kBins; i += kSampThreads) L.hist[i] = 0;
  __syncthreads();
  const int shift = level == 0 ? 21 : level == 1 ? 10 : 0, up = level == 1 ? 21 : 10;
  const uint32_t mask = level == 2 ? 0x3FFu : 0x7FFu;
  sweep(sc, V, vec4, [&](int, float s) {
    const uint32_t k = score_key(s);
    if (level == 0 || (k >> up) == (prefix >> up)) { const u64 w = weight(s, k); if (w) atomicAdd(&L.hist[(k >> shift) & mask], w); }
  });
  __syncthreads();
}

// The smallest 32-bit key t with weight{key > t} < limit, by three radix levels.  PREFILLED: L.hist must already hold the first
// level, as radix_fill(level 0, weight) leaves it (top-k fuses those sums into the row-max sweep; top-p fills it to take Z from
// its total before it knows `limit`) -- levels 1 and 2 are filled here.
template <typename W>
__device__ __forceinline__ uint32_t radix_select_prefilled(const RadixLds& L, const float* sc, int V, int vec4, u64 limit, W weight) {
  uint32_t prefix = 0;
  u64 above = 0;
#pragma unroll
  for (int level = 0; level < 3; ++level) {
    if (level > 0) radix_fill(L, sc, V, vec4, level, prefix, weight);
    descend(L, above, limit);
    prefix |= (uint32_t)*L.digit << (level == 0 ? 21 : level == 1 ? 10 : 0);
    above = *L.above;
    __syncthreads();
  }
  return prefix;
}

__global__ __launch_bounds__(kSampThreads) void sample_step_kernel(SampleArgs p) {
  __shared__ u64 s_hist[kBins];
  __shared__ u64 s_wtot[kSampWaves];
  __shared__ u64 s_above, s_incl;
  __shared__ float s_wmax[kSampWaves];
  __shared__ float s_wmin[kSampWaves];
  __shared__ int s_wcnt[kSampWaves];
  __shared__ int s_digit, s_tok;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int row = blockIdx.x, V = p.V;
  if (*p.unfinished == 0) return;                 // the look-ahead loop's speculative launch past the end: nothing to do
  const long long cur_ll = *p.cur;
  if (cur_ll < 0 || cur_ll >= p.max_new) return;  // (never on the product path: *unfinished is 0 once cur reaches max_new)
  const int cur = (int)cur_ll;
  const float* lg = p.logits + (size_t)row * V;
  float* sc = p.score + (size_t)row * V;
  const int vec4 = p.vec4;

  // ---- pass A: scores = logits / temperature, then the penalised history and the EOS ids patched in place --------------------
  {
    const float T = p.temperature;
    const bool div = T != 1.0f;
    if (vec4) {
      const int n4 = V >> 2;
      const float4* r4 = (const float4*)lg;
      float4* w4 = (float4*)sc;
      for (int base = tid; base < n4; base += kSampThreads * 8) {
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = base + j * kSampThreads;
          if (i < n4) v[j] = r4[i];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = base + j * kSampThreads;
          if (i < n4) {
            float4 o = v[j];
            if (div) { o.x /= T; o.y /= T; o.z /= T; o.w /= T; }
            o.x = o.x == 0.f ? 0.f : o.x; o.y = o.y == 0.f ? 0.f : o.y; o.z = o.z == 0.f ? 0.f : o.z; o.w = o.w == 0.f ? 0.f : o.w;
            w4[i] = o;
          }
        }
      }
    } else {
      for (int i = tid; i < V; i += kSampThreads) {
        float o = div ? lg[i] / T : lg[i];
        sc[i] = o == 0.f ? 0.f : o;
      }
    }
    __syncthreads();
    const long long* hist_tok = p.seq + (size_t)row * p.max_new;
    if (p.rep_pen != 1.0f) {
      for (int t = tid; t < cur; t += kSampThreads) {
        const long long ix = hist_tok[t];
        if (ix < 0 || ix >= V) continue;          // a fill token outside the vocabulary has no logit to penalise
        float g = lg[ix];
        g = g < 0.f ? g * p.rep_pen : g / p.rep_pen;
        if (div) g /= T;
        sc[ix] = g == 0.f ? 0.f : g;
      }
      __syncthreads();
    }
    // NoRepeatNGram: every earlier window that equals the last n - 1 tokens bans the token that followed it (include/mxvl.h)
    const int n = p.ngram;
    if (n > 0 && cur >= n) {                      // cur < n: no window start i <= cur - n (covers HF's cur + 1 < n and cur + 1 == n)
      for (int i = tid; i <= cur - n; i += kSampThreads) {
        bool same = true;
        for (int j = 0; j < n - 1 && same; ++j) same = hist_tok[i + j] == hist_tok[cur - n + 1 + j];
        const long long w = hist_tok[i + n - 1];
        if (same && w >= 0 && w < V) sc[w] = -__builtin_inff();
      }
      __syncthreads();
    }
    if (cur < p.min_new && tid < p.n_eos) {
      const long long e = p.eos[tid];
      if (e >= 0 && e < V) sc[e] = -__builtin_inff();
    }
    __syncthreads();
  }

  // ---- pass 1: row max (+ first radix level of top-k) ----------------------------------------------------------------------------
  const bool use_k = p.top_k > 0 && p.top_k < V, use_p = p.top_p < 1.0f;
  for (int i = tid; i < kBins; i += kSampThreads) s_hist[i] = 0;
  __syncthreads();
  float mx = -__builtin_inff();
  if (use_k) sweep(sc, V, vec4, [&](int, float s) { mx = fmaxf(mx, s); atomicAdd(&s_hist[score_key(s) >> 21], (u64)1); });
  else sweep(sc, V, vec4, [&](int, float s) { mx = fmaxf(mx, s); });
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, kWave));
  if (lane == 0) s_wmax[wave] = mx;
  __syncthreads();
  mx = s_wmax[0];
#pragma unroll
  for (int w = 1; w < kSampWaves; ++w) mx = fmaxf(mx, s_wmax[w]);

  // ---- top-k: the k-th largest key -------------------------------------------------------------------------------------------------
  const RadixLds L = {s_hist, s_wtot, &s_above, &s_incl, &s_digit};
  uint32_t key_min = 0;                           // kept <=> key >= key_min
  if (use_k) key_min = radix_select_prefilled(L, sc, V, vec4, (u64)p.top_k, [](float, uint32_t) -> u64 { return 1; });

  // mass of a kept score in units of 2^-qbits (truncated): an integer, so sums of it do not depend on their order
  const float mscale = p.mass_scale;
  auto mass = [&](float s) -> u64 { return (u64)(fast_exp2((s - mx) * kLog2e) * mscale); };

  // ---- top-p: the smallest key t with mass{key > t} < top_p * Z, a mass per bucket instead of a count --------------------------
  if (use_p) {
    auto kept_mass = [&](float s, uint32_t k) -> u64 { return k >= key_min ? mass(s) : 0; };
    radix_fill(L, sc, V, vec4, 0, 0u, kept_mass);
    const u64 Z = hist_total(L);
    // top_p * Z, rounded up: mass{key > t} is an integer, so `< top_p * Z` is `< ceil(top_p * Z)`
    const double pz = (double)p.top_p * (double)Z;
    u64 limit = (u64)pz;
    if ((double)limit < pz) ++limit;
    if (limit == 0) limit = 1;                    // the largest score is always kept
    const uint32_t t = radix_select_prefilled(L, sc, V, vec4, limit, kept_mass);
    key_min = t > key_min ? t : key_min;
  }

  // ---- final: kept mass of the 16 contiguous parts (wave w owns blocks of 256 tokens [w * bpw, (w + 1) * bpw)), then the draw ----
  const int nblk = (V + 255) >> 8, bpw = (nblk + kSampWaves - 1) / kSampWaves;
  const int blk0 = wave * bpw, blk1 = (blk0 + bpw < nblk) ? blk0 + bpw : nblk;
  auto load4 = [&](int blk, float (&v)[4]) {       // tokens blk * 256 + lane * 4 + {0..3}; -inf (mass 0, never kept) past the row
    const int i0 = blk * 256 + lane * 4;
    if (vec4 && i0 + 3 < V) { const float4 q = *(const float4*)(sc + i0); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (i0 + e < V) ? sc[i0 + e] : __builtin_nanf("");
    }
  };
  // (a NaN marks "past the row": its key compare is skipped explicitly below)
  u64 part = 0;
  int cnt = 0;
  float mn = __builtin_inff();
  for (int b0 = blk0; b0 < blk1; b0 += 8) {
    float v[8][4];
#pragma unroll
    for (int j = 0; j < 8; ++j) if (b0 + j < blk1) load4(b0 + j, v[j]);
#pragma unroll
    for (int j = 0; j < 8; ++j) if (b0 + j < blk1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float s = v[j][e];
        const bool in_row = (b0 + j) * 256 + lane * 4 + e < V;
        if (in_row && score_key(s) >= key_min) { part += mass(s); ++cnt; mn = fminf(mn, s); }
      }
    }
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    part += __shfl_xor(part, d, kWave);
    cnt += __shfl_xor(cnt, d, kWave);
    mn = fminf(mn, __shfl_xor(mn, d, kWave));
  }
  if (lane == 0) { s_wtot[wave] = part; s_wcnt[wave] = cnt; s_wmin[wave] = mn; }
  if (tid == 0) s_tok = -1;
  __syncthreads();
  u64 Zk = 0;
  for (int w = 0; w < kSampWaves; ++w) Zk += s_wtot[w];
  const u64 seed = (u64)*p.seed;
  const u64 U = sample_hash(seed, (uint32_t)row, (uint32_t)cur) >> 8;                  // u = U * 2^-24
  // floor(U * Zk / 2^24) from the 128-bit product: cum > u * Zk  <=>  cum > target (cum is an integer); target < Zk since U < 2^24
  const u64 target = (__umul64hi(U, Zk) << 40) | ((U * Zk) >> 24);
  u64 before = 0;
  int wsel = -1;
  for (int w = 0; w < kSampWaves; ++w) {
    if (wsel < 0 && before + s_wtot[w] > target) wsel = w;
    if (wsel < 0) before += s_wtot[w];
  }
  if (wave == wsel) {                             // one wave walks its part in index order
    u64 carry = before;
    bool found = false;
    for (int b0 = blk0; b0 < blk1 && !found; b0 += 8) {
      float v[8][4];
#pragma unroll
      for (int j = 0; j < 8; ++j) if (b0 + j < blk1) load4(b0 + j, v[j]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (found || b0 + j >= blk1) continue;    // wave-uniform
        u64 m[4];
        u64 ls = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool in_row = (b0 + j) * 256 + lane * 4 + e < V;
          m[e] = (in_row && score_key(v[j][e]) >= key_min) ? mass(v[j][e]) : 0;
          ls += m[e];
        }
        const u64 inc = wave_incl_scan(ls);
        const u64 tot = __shfl(inc, kWave - 1, kWave);
        if (carry + tot > target) {
          u64 c = carry + inc - ls;               // cumulative mass in front of this lane's four tokens
          if (c <= target && c + ls > target) {   // exactly one lane
            int e = 0;
            while (e < 3 && c + m[e] <= target) { c += m[e]; ++e; }
            s_tok = (b0 + j) * 256 + lane * 4 + e;
          }
          found = true;
        } else {
          carry += tot;
        }
      }
    }
  }
  __syncthreads();

  // ---- bookkeeping of the row, then the rows meet ------------------------------------------------------------------------------------
  if (tid == 0) {
    int kept = 0;
    float thr = __builtin_inff();
    for (int w = 0; w < kSampWaves; ++w) { kept += s_wcnt[w]; thr = fminf(thr, s_wmin[w]); }
    if (p.out_thresh) p.out_thresh[row] = thr;
    if (p.out_kept) p.out_kept[row] = kept;
    int drawn = s_tok;
    if (drawn < 0 || drawn >= V) drawn = 0;       // unreachable with finite logits (Zk > target): keeps the id inside the vocabulary
    const bool was_alive = p.alive[row] != 0;
    const long long tk = was_alive ? (long long)drawn : p.fill;
    bool is_eos = false;
    for (int e = 0; e < p.n_eos; ++e) is_eos = is_eos || (p.eos[e] == tk);
    const bool now_alive = was_alive && !is_eos;
    p.tok[row] = tk;
    p.seq[(size_t)row * p.max_new + cur] = tk;
    p.alive[row] = now_alive ? 1 : 0;
    bool last = true;
    unsigned int n_alive = now_alive ? 1u : 0u;
    if (gridDim.x > 1) {
      const unsigned int inc = 1u | (now_alive ? 1u << 8 : 0u);
      const unsigned int tot = atomicAdd(p.ticket, inc) + inc;
      last = (tot & 0xffu) == gridDim.x;
      n_alive = (tot >> 8) & 0xffu;
      if (last) atomicExch(p.ticket, 0u);
    }
    if (last) {       // every workgroup read *cur and *unfinished at its start, before it arrived
      const bool unf = n_alive != 0 && cur + 1 < p.max_new;
      *p.unfinished = unf ? 1 : 0;
      if (p.unf_log) __hip_atomic_store(p.unf_log + cur, (unsigned char)(unf ? 1 : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      *p.cur = (long long)cur + 1;
    }
  }
}

}  // namespace mxvl

using namespace mxvl;

extern "C" int64_t mxvl_sample_workspace_bytes(int rows, int vocab) {
  if (rows <= 0 || vocab <= 0) return 0;
  return 4 * (int64_t)rows * (((int64_t)vocab + 3) & ~(int64_t)3);
}

extern "C" int mxvl_sample_step(const mxvl_sample_desc* d, void* hip_stream) {
  if (!d) return MXVL_ERR_NULL;
  if (d->rows <= 0 || d->rows > kSampMaxRows || d->vocab <= 0 || d->max_new <= 0 || d->min_new < 0 || d->n_eos < 0 || d->n_eos > kSampMaxEos ||
      d->top_k < 0 || d->no_repeat_ngram_size < 0 || (long long)d->rows * d->vocab > 0x7fffffffLL)
    return MXVL_ERR_SHAPE;
  if (!(d->temperature > 0.f) || !(d->temperature < __builtin_inff()) || !(d->top_p > 0.f) || !(d->top_p <= 1.f) ||
      !(d->repetition_penalty > 0.f))
    return MXVL_ERR_SHAPE;
  if (!d->workspace || d->workspace_bytes < mxvl_sample_workspace_bytes(d->rows, d->vocab)) return MXVL_ERR_SHAPE;
  if (!d->logits || !d->seq || !d->alive || !d->tok || !d->cur || !d->seed || !d->unfinished || (d->rows > 1 && !d->scratch))
    return MXVL_ERR_NULL;
  if (d->n_eos > 0 && !d->eos) return MXVL_ERR_NULL;
  SampleArgs a;
  a.rows = d->rows; a.V = d->vocab; a.max_new = d->max_new; a.min_new = d->min_new; a.n_eos = d->n_eos; a.top_k = d->top_k;
  a.ngram = d->no_repeat_ngram_size;
  a.rep_pen = d->repetition_penalty; a.temperature = d->temperature; a.top_p = d->top_p; a.fill = d->fill;
  // mass unit 2^-qbits: the sum of `vocab` masses <= 1 stays below 2^62
  int lg = 0;
  while ((1LL << lg) < (long long)d->vocab) ++lg;
  const int qbits = 62 - lg < 40 ? 62 - lg : 40;
  a.mass_scale = ldexpf(1.0f, qbits);
  a.logits = (const float*)d->logits; a.score = (float*)d->workspace;
  a.seq = (long long*)d->seq; a.alive = (unsigned char*)d->alive; a.tok = (long long*)d->tok; a.cur = (long long*)d->cur;
  a.eos = (const long long*)d->eos; a.seed = (const long long*)d->seed;
  a.unfinished = (unsigned char*)d->unfinished; a.unf_log = (unsigned char*)d->unfinished_log;
  a.ticket = (unsigned int*)d->scratch;
  a.out_thresh = (float*)d->out_thresh; a.out_kept = (int*)d->out_kept;
  a.vec4 = (a.V % 4 == 0 && ((uintptr_t)a.logits & 15) == 0 && ((uintptr_t)a.score & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(sample_step_kernel, dim3(d->rows), dim3(kSampThreads), 0, (hipStream_t)hip_stream, a);
  return launch_status();
}
