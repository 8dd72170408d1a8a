// decode_gemm.hip -- host side of the 9..80-row decoder projections (kernels: decode_gemm.h) and of mxvl_decode_rmsnorm.
// mxvl_decode_gemv (decode.hip) forwards here for rows > 8, so the stepper has ONE projection entry for every row count the
// reference's launch scripts decode at (MambaXrayVL_DownStream.py:292-301; 3 .. 80 rows).
#include <initializer_list>
#include "decode_gemm.h"

namespace mxvl {

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
// K % 64 == 0 (every real decoder: 4096 / 11008 / 3584 / 18944): LDS-DMA weight stream, 4 waves x R tiles, two workgroups per CU.
template <typename E, int MT, int R, int NW, int PF>
static int launch_dma(const DecodeGemmArgs& a, int splits, hipStream_t s) {
  const int cols_per_wg = (a.swiglu ? R / 2 : R) * 16;
  const dim3 grid((a.N + cols_per_wg - 1) / cols_per_wg, splits);
  const size_t ring = (size_t)NW * PF * R * 2048, red = (size_t)NW * 2 * MT * 1024 + (a.g ? (size_t)NW * MT * 64 : 0);
  const size_t lds = ring > red ? ring : red;
  // NORM needs (PF - 1) * (OPS + 2) <= 63 outstanding operations: the ring is one stage shallower where it would not fit
  constexpr bool norm_fits = (PF - 1) * (2 * R + 2 * MT + 2) <= 63;
  void (*kern)(const DecodeGemmArgs) = decode_gemm_dma_kernel<E, MT, R, NW, PF>;
  if (a.g) {
    if constexpr (norm_fits) kern = decode_gemm_dma_kernel<E, MT, R, NW, PF, true>;
    else kern = decode_gemm_dma_kernel<E, MT, R, NW, (PF > 2 ? PF - 1 : 2), true>;
  }
  if (lds > 64 * 1024 && hip_status(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != MXVL_OK)
    return MXVL_ERR_LAUNCH;   // per call: the attribute is per device
  hipLaunchKernelGGL(kern, grid, dim3(NW * 64), lds, s, a);
  return launch_status();
}

// any K % 8 == 0: fragments loaded straight into the MFMA operands
template <typename E, int MT, int R>
static int launch_direct(const DecodeGemmArgs& a, int splits, hipStream_t s) {
  constexpr int NW = 8, PF = (R + MT <= 4) ? 4 : ((R + MT <= 6) ? 3 : 2);
  const int cols_per_wg = (a.swiglu ? R / 2 : R) * 16;
  const dim3 grid((a.N + cols_per_wg - 1) / cols_per_wg, splits);
  const size_t lds = (size_t)NW * 2 * MT * 1024;
  auto kern = decode_gemm_kernel<E, MT, R, NW, PF>;
  if (lds > 64 * 1024 && hip_status(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != MXVL_OK)
    return MXVL_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, grid, dim3(NW * 64), lds, s, a);
  return launch_status();
}

// ---- the N-split ring kernels (decode_gemm.h dg_nsplit_body): 16-bit weights at 17..80 rows (decode_gemm_wide_kernel), MXVL_W_INT8
// (decode_gemm_w8_kernel), MXVL_W_FP8 (decode_gemm_w8f_kernel), MXVL_W_MXFP4 (decode_gemm_w4_kernel) and MXVL_W_INT4 (decode_gemm_w4i_kernel)
// at every row count ----------------------------------------------------------------------------------------------------------------
// ring depth: as many stages of `stage` bytes as `budget` bytes of LDS hold (one workgroup per CU is all these grids ask for), capped
// by the 6-bit vmcnt field (`ops` requests per stage) and at 8 -- against the first version's 3 stages: 48-row token +5 %, 80-row
// +0.7 % (profiles/r05_decode_gemm_ring_ab.txt)
constexpr int ring_depth(int stage, int ops, int budget) {
  int pf = budget / stage;
  while (pf > 2 && (pf - 1) * ops > 63) --pf;
  return pf > 8 ? 8 : (pf < 2 ? 2 : pf);
}
// a stage: IMGS activation images of MT tiles + NW x R weight tiles, 2 R + ceil(2 IMGS MT / NW) requests per wave; the LDS budgets
// (Fmt::RING_BYTES) stand beside the format traits in decode_gemm.h
template <typename Fmt> constexpr int nsplit_stage(int MT, int R, int NW) { return Fmt::IMGS * MT * 2048 + NW * R * 2048; }
template <typename Fmt> constexpr int nsplit_pf(int MT, int R, int NW) {
  return ring_depth(nsplit_stage<Fmt>(MT, R, NW), 2 * R + (2 * Fmt::IMGS * MT + NW - 1) / NW, Fmt::RING_BYTES);
}
template <typename Fmt> static int nsplit_cpw(const DecodeGemmArgs& a, int splits) {      // chunks of a workgroup's K range
  return ((a.K + 64 * Fmt::IMGS - 1) / (64 * Fmt::IMGS) + splits - 1) / splits;
}
static int g_wide_pf3 = 0;     // (A/B: mxvl_set_decode_gemm_wide(3) = the 3-stage ring of the first version)
static int g_wide_nw4 = 0;     // (A/B: mxvl_set_decode_gemm_wide(4) = four waves per workgroup everywhere)
static int g_wide_min_mt = 2;  // wide from 17 rows on (A/B: mode 5 = from 33 rows on, as first shipped; mode 6 = from 1 row on)
static int g_wide_min_g = 64;  // ... for grids of at least 64 workgroups (A/B: mode 5 = 160)
static int g_decode_gemm_wide = 1;        // mxvl_set_decode_gemm_wide: the A/B switch of tools / bench (default on; 2: also at 17..32 rows)

// THE list of weight formats: f(the trait of weight flag `flag`), 0 = 16-bit.  Anything else -- two flags at once -- is no format.
template <typename F>
static int with_format(int flag, F&& f) {
  switch (flag) {
    case DgW16::W_FLAG: return f(DgW16{});
    case DgW8::W_FLAG: return f(DgW8{});
    case DgW4::W_FLAG: return f(DgW4{});
    case DgW8F::W_FLAG: return f(DgW8F{});
    case DgW4I::W_FLAG: return f(DgW4I{});
    default: return MXVL_ERR_DTYPE;
  }
}

template <typename Fmt, typename E, int MT, int R, int NW, int PF>
static int launch_nsplit(const DecodeGemmArgs& a, int splits, hipStream_t s) {
  const int cols_per_wg = NW * (a.swiglu ? R / 2 : R) * 16;
  const dim3 grid((a.N + cols_per_wg - 1) / cols_per_wg, splits);
  const size_t lds = (size_t)PF * nsplit_stage<Fmt>(MT, R, NW) + (size_t)Fmt::scale_lds(NW, R, nsplit_cpw<Fmt>(a, splits));
  void (*kern)(const DecodeGemmArgs);      // the __global__ wrapper of the format (decode_gemm.h): the one place that names them
  if constexpr (std::is_same_v<Fmt, DgW8>) kern = decode_gemm_w8_kernel<E, MT, R, NW, PF>;
  else if constexpr (std::is_same_v<Fmt, DgW8F>) kern = decode_gemm_w8f_kernel<E, MT, R, NW, PF>;
  else if constexpr (std::is_same_v<Fmt, DgW4>) kern = decode_gemm_w4_kernel<E, MT, R, NW, PF>;
  else if constexpr (std::is_same_v<Fmt, DgW4I>) kern = decode_gemm_w4i_kernel<E, MT, R, NW, PF>;
  else kern = decode_gemm_wide_kernel<E, MT, R, NW, PF>;
  if (lds > 64 * 1024 && hip_status(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != MXVL_OK)
    return MXVL_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, grid, dim3(NW * 64), lds, s, a);
  return launch_status();
}

// The N-split kernels' plan for a launch, shared by the launch below and by mxvl_decode_gemm_plan (the dispatch as a pure function
// of the descriptor: tests/test_abi.py pins it for the reference's decoder shapes without a GPU).
// What bounds these launches is what ONE CU can pull through its load path, weights and activations together (~50 GB/s of
// full-line LDS-DMA, tools/cu_stream_probe.hip -- HBM needs 27 GB/s from each of 256 CUs): a workgroup of NW waves x R tiles
// moves 1 + f MT / (NW R) bytes per weight byte (f = 1 / 2 / 4 for 16-bit / int8 / mxfp4 weights: the weight bytes halve, the
// activations do not), and the launch is as long as its busiest CU.  So: of the candidates, the (NW, R) with the least
//   (1 + f MT / (NW R)) x rounds / workgroups,      rounds = ceil(workgroups / 256)   (the LDS ring leaves one workgroup per CU)
// -- three waves per workgroup when that fills the chip: 230 workgroups for Llama's gate / up (172 with four waves), 256 for qkv (192).
// (For f = 2, 4 a starting point: the 16-bit kernels' model, not a measurement of half- and quarter-size tiles.)
struct WidePlan { int nw, r; long g; };
template <typename Fits>
static WidePlan nsplit_plan(int f, int MT, const DecodeGemmArgs& a, int splits, std::initializer_list<WidePlan> cands, Fits fits) {
  WidePlan pl{0, 0, 0};
  double best = 1e30;
  for (const WidePlan& c : cands) {
    if ((a.swiglu && (c.r & 1)) || !fits(c)) continue;
    const int cols = c.nw * (a.swiglu ? c.r / 2 : c.r) * 16;
    const long g = (long)((a.N + cols - 1) / cols) * splits;
    const double est = (1.0 + (double)(f * MT) / (c.nw * c.r)) * (double)((g + 255) / 256) / (double)g;
    if (est < best - 1e-12) { best = est; pl = WidePlan{c.nw, c.r, g}; }
  }
  return pl;
}
// kind of the launch as mxvl_decode_gemm_plan reports it: Fmt::KIND (1 / 3 / 4 / 5 / 6 = the 16-bit / int8 / mxfp4 / fp8 / int4 N-split kernel)
// with `pl`, 0 = the K-split kernels keep it, < 0 = an error.  Three planning groups, by the bytes a weight takes (Fmt::IMGS).
template <typename Fmt>
static int decode_plan(int MT, const DecodeGemmArgs& a, int splits, WidePlan& pl) {
  // quantised: four waves, one or two tiles per wave (four leave the ring two or three stages at 33..80 rows and no registers for
  // the widened operands)
  if constexpr (Fmt::IMGS == 2) {     // int8 and fp8 move the same bytes through the same geometry: one plan
    pl = nsplit_plan(Fmt::IMGS, MT, a, splits, {{4, 1}, {4, 2}}, [](const WidePlan&) { return true; });
    return Fmt::KIND;
  } else if constexpr (Fmt::IMGS == 4) {     // mxfp4 and int4 move the same bytes (codes and K / 32 scale bytes per row) through the same geometry: one plan.
                  // the scale rows' share of LDS: two tiles per wave up to a K range of 12032 columns per workgroup, one tile up to 24320
    const int cpw = nsplit_cpw<Fmt>(a, splits);
    pl = nsplit_plan(Fmt::IMGS, MT, a, splits, {{4, 1}, {4, 2}}, [&](const WidePlan& c) { return Fmt::scale_lds(c.nw, c.r, cpw) <= kW4ScaleBytes; });
    return pl.r ? Fmt::KIND : MXVL_ERR_UNSUPPORTED;
  } else {
    // 16-bit: from 17 rows and 64 workgroups on (profiles/r05_decode_gemm_wide_rows_ab.txt: against the K-split kernels the 18-row token
    // +7 %, the 24-row token +11 %, Qwen1.5-1.8B's 96..128-workgroup projections +4 % at 80 rows; the first version -- 3-stage
    // ring, aligned walks -- had lost to them below 160 workgroups and at 17..32 rows).  At 1..16 rows the K-split kernel keeps the
    // launches: it carries the fused RMSNorm, and without it the wide kernel is +2 % (Llama) / 0 % (Qwen) there.
    if (!(g_decode_gemm_wide && MT >= g_wide_min_mt && a.K % Fmt::K_MULT == 0 && a.K >= 256 && !a.g)) return 0;
    pl = nsplit_plan(Fmt::IMGS, MT, a, splits, {{4, 1}, {4, 2}, {4, 4}, {3, 1}, {3, 2}}, [](const WidePlan& c) { return c.nw == 4 || !g_wide_nw4; });
    return pl.g >= g_wide_min_g ? Fmt::KIND : 0;
  }
}
// ring depth of a planned launch (the 3-stage A/B ring is a 16-bit mode)
template <typename Fmt> static int plan_pf(int MT, const WidePlan& pl) {
  return Fmt::IMGS == 1 && pl.nw == 4 && g_wide_pf3 ? 3 : nsplit_pf<Fmt>(MT, pl.r, pl.nw);
}

template <typename Fmt, typename E, int MT, int R, int NW>
static int launch_nsplit_r(const DecodeGemmArgs& a, int splits, hipStream_t s) {
  if constexpr (Fmt::IMGS == 1 && NW == 4) { if (g_wide_pf3) return launch_nsplit<Fmt, E, MT, R, 4, 3>(a, splits, s); }
  return launch_nsplit<Fmt, E, MT, R, NW, nsplit_pf<Fmt>(MT, R, NW)>(a, splits, s);
}
template <typename Fmt, typename E, int MT>
static int launch_planned(const WidePlan& pl, const DecodeGemmArgs& a, int splits, hipStream_t s) {
  if constexpr (Fmt::IMGS == 1) {       // the geometries only the 16-bit plan proposes
    if (pl.nw == 3) return pl.r == 2 ? launch_nsplit_r<Fmt, E, MT, 2, 3>(a, splits, s) : launch_nsplit_r<Fmt, E, MT, 1, 3>(a, splits, s);
    if (pl.r == 4) return launch_nsplit_r<Fmt, E, MT, 4, 4>(a, splits, s);
  }
  return pl.r == 2 ? launch_nsplit_r<Fmt, E, MT, 2, 4>(a, splits, s) : launch_nsplit_r<Fmt, E, MT, 1, 4>(a, splits, s);
}

template <typename E, int MT>
static int launch_decode_gemm(const DecodeGemmArgs& a, int splits, hipStream_t s) {
  int kind = 0;
  const int planned = with_format(a.w_flag, [&](auto fmt) -> int {
    WidePlan pl;
    kind = decode_plan<decltype(fmt)>(MT, a, splits, pl);
    return kind > 0 ? launch_planned<decltype(fmt), E, MT>(pl, a, splits, s) : kind;
  });
  if (kind != 0 || planned != MXVL_OK) return planned;      // launched, or refused; kind 0: the K-split kernels below
  // R = weight tiles per workgroup.  Two effects, both measured (tools/decode_gemm_bench.py A/B at 18 rows, profiles/r04_decode_gemm_r_sweep.txt):
  // (1) a CU streams ~28 GB/s whatever it holds, so the workgroups must fill whole rounds of the 256 CUs -- 344 workgroups (gate / up
  //     at R = 4: 88 CUs with two, 168 with one) run at 4.7 TB/s, 688 (R = 2) at 5.3, 256 (qkv at R = 3) at 5.2 against 4.3 for 384;
  // (2) the activation re-read from L2 per weight byte is MT / R: at equal fill R = 4 beats R = 2 by 6 % (lm_head 5.73 vs 5.37 TB/s).
  // score = fill of the last round x 1 / (1 + 0.06 MT / R); SwiGLU needs an even R (gate and up tiles of the same columns).
  const int tiles = (a.N + 15) / 16;
  auto score = [&](int R) {
    const long wgs = (long)(a.swiglu ? (tiles + R / 2 - 1) / (R / 2) : (tiles + R - 1) / R) * splits;
    const long rounds = (wgs + 255) / 256;
    return (double)wgs / (double)(rounds * 256) / (1.0 + 0.06 * MT / R);
  };
  if (a.K % 64 == 0 && a.K >= 256) {
    constexpr int PFN = MT <= 2 ? 4 : 2;       // narrow workgroups: deeper rings while the activation fragments fit the registers
    int best = a.swiglu ? 2 : 1;
    for (int R : {2, 3, 4}) {
      if (a.swiglu && (R & 1)) continue;
      if (score(R) > score(best) + 1e-9) best = R;
    }
    switch (best) {
      case 4: return launch_dma<E, MT, 4, 4, 2>(a, splits, s);
      case 3: return launch_dma<E, MT, 3, 4, 2>(a, splits, s);
      case 2: return launch_dma<E, MT, 2, 4, PFN>(a, splits, s);
      default: return launch_dma<E, MT, 1, 8, PFN>(a, splits, s);
    }
  }
  if (a.swiglu) return tiles >= 768 ? launch_direct<E, MT, 4>(a, splits, s) : launch_direct<E, MT, 2>(a, splits, s);
  if (tiles >= 1536) return launch_direct<E, MT, 4>(a, splits, s);
  if (tiles >= 512) return launch_direct<E, MT, 2>(a, splits, s);
  return launch_direct<E, MT, 1>(a, splits, s);
}

template <typename E>
static int launch_decode_gemm_rows(const DecodeGemmArgs& a, int splits, hipStream_t s) {
  switch ((a.rows + 15) / 16) {
    case 1: return launch_decode_gemm<E, 1>(a, splits, s);
    case 2: return launch_decode_gemm<E, 2>(a, splits, s);
    case 3: return launch_decode_gemm<E, 3>(a, splits, s);
    case 4: return launch_decode_gemm<E, 4>(a, splits, s);
    default: return launch_decode_gemm<E, 5>(a, splits, s);
  }
}

static int decode_gemm_args(const mxvl_gemv_desc* d, DecodeGemmArgs& a, int& splits);

int decode_gemm_dispatch(const mxvl_gemv_desc* d, hipStream_t s) {
  DecodeGemmArgs a;
  int splits = 1;
  const int chk = decode_gemm_args(d, a, splits);
  if (chk != MXVL_OK) return chk;
  return decode_dtype(d->dtype & ~kWeightFlags) == MXVL_F16 ? launch_decode_gemm_rows<EltF16>(a, splits, s) : launch_decode_gemm_rows<EltBf16>(a, splits, s);
}

// out: kind (decode_plan), then waves, tiles per wave, ring stages, workgroups of the N-split kernel; kind 0: zeros
int decode_gemm_plan(const mxvl_gemv_desc* d, int32_t* out) {
  DecodeGemmArgs a;
  int splits = 1;
  const int chk = decode_gemm_args(d, a, splits);
  if (chk != MXVL_OK) return chk;
  const int MT = (a.rows + 15) / 16 > 5 ? 5 : (a.rows + 15) / 16;
  return with_format(a.w_flag, [&](auto fmt) -> int {
    WidePlan pl;
    const int kind = decode_plan<decltype(fmt)>(MT, a, splits, pl);
    if (kind < 0) return kind;
    if (kind == 0) pl = WidePlan{0, 0, 0};
    out[0] = kind; out[1] = pl.nw; out[2] = pl.r; out[4] = (int32_t)pl.g;
    out[3] = kind == 0 ? 0 : plan_pf<decltype(fmt)>(MT, pl);
    return MXVL_OK;
  });
}

// argument checks of mxvl_decode_gemv + the kernel-side argument block (nothing is launched here)
static int decode_gemm_args(const mxvl_gemv_desc* d, DecodeGemmArgs& a, int& splits) {
  if (!decode_dtype_ok(d->dtype & ~kWeightFlags)) return MXVL_ERR_DTYPE;
  a.w_flag = d->dtype & kWeightFlags;
  a.ws = a.ws2 = nullptr;
  a.wx = a.wx2 = nullptr;
  const int chk = with_format(a.w_flag, [&](auto fmt) -> int {      // one weight format at most: two flags are MXVL_ERR_DTYPE
    using Fmt = decltype(fmt);
    constexpr bool quantised = Fmt::W_FLAG != 0;                    // w_scale / w2_scale exist in the caller's struct only behind a flag
    if constexpr (quantised) { if (!d->w_scale || (d->swiglu && !d->w2_scale)) return MXVL_ERR_NULL; }
    if (d->rows <= 0 || d->rows > 80 || d->K < 32 || d->N <= 0) return MXVL_ERR_SHAPE;
    if constexpr (quantised) {                                      // whole Fmt::K_MULT columns; no quantised form of the fused norm and the fp32 logits
      if (d->K % Fmt::K_MULT != 0 || d->K < Fmt::K_MULT || d->norm_weight || d->out_f32) return MXVL_ERR_SHAPE;
      Fmt::set_scales(a, d->w_scale, d->swiglu ? d->w2_scale : nullptr);
    }
    return MXVL_OK;
  });
  if (chk != MXVL_OK) return chk;
  if (d->K % 8 != 0) return MXVL_ERR_UNSUPPORTED;                      // 16-byte fragments
  if (d->swiglu && (!d->W2 || d->out_f32)) return MXVL_ERR_UNSUPPORTED;
  // RMSNorm fused into the projection (ABI v8): the LDS-DMA kernel only (K % 64 == 0); elsewhere rows come from mxvl_decode_rmsnorm
  if (d->norm_weight && (d->K % 64 != 0 || d->K < 256 || d->split_acc)) return MXVL_ERR_UNSUPPORTED;
  if ((long long)d->N * d->K > 0x7fffffffLL * 16) return MXVL_ERR_SHAPE;
  a.rows = d->rows; a.K = d->K; a.N = d->N; a.swiglu = d->swiglu; a.out_f32 = d->out_f32;
  a.x = (const uint16_t*)d->x; a.W = (const uint16_t*)d->W; a.W2 = (const uint16_t*)d->W2;
  a.bias = (const uint16_t*)d->bias; a.res = (const uint16_t*)d->residual; a.y = d->y;
  a.split_acc = (float*)d->split_acc;
  a.g = (const uint16_t*)d->norm_weight; a.eps = d->eps;
  a.g_scale = 1.0f; a.g_inv = 1.0f;
  if (d->norm_weight && d->norm_gain_scale != 0.0f) {
    int e = 0;
    const float m = frexpf(d->norm_gain_scale, &e);
    if (m != 0.5f || e < -60 || e > 60) return MXVL_ERR_UNSUPPORTED;    // a positive power of two, or nothing
    a.g_scale = d->norm_gain_scale; a.g_inv = 1.0f / d->norm_gain_scale;
  }
  splits = 1;
  if (!a.split_acc && d->k_splits > 1) return MXVL_ERR_UNSUPPORTED;    // a split needs the accumulator
  if (a.split_acc) {        // the caller folds the fp32 sums itself (mxvl_decode_rmsnorm): no epilogue here
    if (d->swiglu || d->bias || d->residual || d->out_f32 || d->k_splits < 1 || d->k_splits > 16) return MXVL_ERR_UNSUPPORTED;
    splits = d->k_splits;
  }
  return MXVL_OK;
}

}  // namespace mxvl

using namespace mxvl;

extern "C" int mxvl_decode_rmsnorm(const mxvl_rmsnorm_desc* d, void* hip_stream) {
  if (!d || !d->weight || !d->y) return MXVL_ERR_NULL;
  if (d->acc ? (!d->residual || !d->x_out) : !d->x) return MXVL_ERR_NULL;
  if (!decode_dtype_ok(d->dtype)) return MXVL_ERR_DTYPE;
  if (d->rows <= 0 || d->K <= 0) return MXVL_ERR_SHAPE;
  if (d->K % 8 != 0 || d->K > 16384) return MXVL_ERR_UNSUPPORTED;
  RmsNormArgs a;
  a.rows = d->rows; a.K = d->K; a.eps = d->eps;
  a.splits = d->acc_splits > 0 ? d->acc_splits : 1;
  if (a.splits > 16) return MXVL_ERR_UNSUPPORTED;
  a.x = (const uint16_t*)d->x; a.g = (const uint16_t*)d->weight; a.y = (uint16_t*)d->y;
  a.acc = (float*)d->acc; a.res = (const uint16_t*)d->residual; a.x_out = (uint16_t*)d->x_out;
  const bool f16 = decode_dtype(d->dtype) == MXVL_F16;
  const dim3 grid(d->rows), block(1024);
  hipStream_t s = (hipStream_t)hip_stream;
#define MXVL_RMSNORM(SS) do { if (f16) hipLaunchKernelGGL((decode_rmsnorm_kernel<EltF16, SS>), grid, block, 0, s, a); \
                              else hipLaunchKernelGGL((decode_rmsnorm_kernel<EltBf16, SS>), grid, block, 0, s, a); } while (0)
  switch (a.acc ? a.splits : 1) {
    case 1: MXVL_RMSNORM(1); break;
    case 2: MXVL_RMSNORM(2); break;
    case 4: MXVL_RMSNORM(4); break;
    case 8: MXVL_RMSNORM(8); break;
    default: MXVL_RMSNORM(0); break;
  }
#undef MXVL_RMSNORM
  return launch_status();
}

/* diagnostic / A-B switch (tools, bench.py --decode-gemm): 0 = the K-split kernels at every row count (round 4), 1 = waves split N with
 * LDS-shared activations at 17..80 rows for grids of >= 64 workgroups (default; 2 = the same), 3 = the wide kernel as first measured
 * (33..80 rows, >= 160 workgroups, 3-stage ring, four waves per workgroup), 4 = as 1 with four waves per workgroup everywhere,
 * 5 = as 1 at 33..80 rows and >= 160 workgroups only, 6 = as 1 from one row on */
extern "C" int mxvl_set_decode_gemm_wide(int on) {
  static int mode = 1;
  const int was = mode;
  mode = on < 0 ? 0 : on;
  mxvl::g_wide_pf3 = on == 3;
  mxvl::g_wide_nw4 = on == 3 || on == 4;
  mxvl::g_wide_min_g = (on == 3 || on == 5) ? 160 : 64;
  mxvl::g_wide_min_mt = (on == 3 || on == 5) ? 3 : (on == 6 ? 1 : 2);
  mxvl::g_decode_gemm_wide = on <= 0 ? 0 : 1;
  return was;
}
