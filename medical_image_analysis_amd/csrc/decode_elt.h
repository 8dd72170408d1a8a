// decode_elt.h -- the 16-bit element type of the decoder-step kernels (decode.hip, decode_gemm.h) as a trait, gfx950 only.
//
// The reference loads its report LLM with torch_dtype=torch.float16 (CXPMRG_Bench_MambaXray_VL/models/MambaXrayVL_DownStream.py:
// 72, 85, 92) and the round-1..4 decode kernels were bf16-only, so the reference's own checkpoint dtype could not decode on them.
// Every kernel of the step is now a template over one of the two traits below; what differs between them is exactly
//   f(v)      the element's value as fp32,
//   r(x)      fp32 -> element bits, round-to-nearest-even (fp16: overflow to inf, as torch's .half()),
//   rr(x)     x rounded through the element type (the rounding points of the modules' 16-bit tensor ops),
//   dot2      v_dot2_f32_bf16 / v_dot2_f32_f16,
//   mfma32    v_mfma_f32_16x16x32_bf16 / _f16   (8 elements per lane),
//   mfma16    v_mfma_f32_16x16x16_bf16 / _f16   (4 elements per lane),
// the memory layout, the LDS-DMA rings, the transpose reads (ds_read_b64_tr_b16 moves 16-bit lanes whatever they mean) and every
// wait count are the same instruction streams.
#pragma once
#include "mxvl_common.h"

namespace mxvl {

typedef float elt_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int elt_u32x4 __attribute__((ext_vector_type(4)));
typedef short elt_s16x4 __attribute__((ext_vector_type(4)));

struct EltBf16 {
  static constexpr int dtype = MXVL_BF16;
  __device__ static inline float f(uint16_t v) { return __builtin_bit_cast(float, (uint32_t)v << 16); }
  __device__ static inline uint16_t r(float x) {
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
  }
  __device__ static inline float rr(float x) { return f(r(x)); }
  // the two elements of a packed word as fp32
  __device__ static inline float lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
  __device__ static inline float hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
  __device__ static inline float dot2(uint32_t a, uint32_t b, float c) {
    typedef short bf16x2_t __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a), __builtin_bit_cast(bf16x2_t, b), c, false);
  }
  __device__ static inline elt_f32x4 mfma32(elt_u32x4 a, elt_u32x4 b, elt_f32x4 c) {
    typedef __bf16 v8 __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
  __device__ static inline elt_f32x4 mfma16(elt_s16x4 a, elt_s16x4 b, elt_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
  }
};

struct EltF16 {
  static constexpr int dtype = MXVL_F16;
  __device__ static inline float f(uint16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
  __device__ static inline uint16_t r(float x) { return __builtin_bit_cast(uint16_t, (_Float16)x); }
  __device__ static inline float rr(float x) { return (float)(_Float16)x; }
  __device__ static inline float lo(uint32_t w) { return f((uint16_t)w); }
  __device__ static inline float hi(uint32_t w) { return f((uint16_t)(w >> 16)); }
  __device__ static inline float dot2(uint32_t a, uint32_t b, float c) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, a), __builtin_bit_cast(h2, b), c, false);
  }
  __device__ static inline elt_f32x4 mfma32(elt_u32x4 a, elt_u32x4 b, elt_f32x4 c) {
    typedef _Float16 v8 __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
  __device__ static inline elt_f32x4 mfma16(elt_s16x4 a, elt_s16x4 b, elt_f32x4 c) {
    typedef _Float16 v4 __attribute__((ext_vector_type(4)));
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(v4, a), __builtin_bit_cast(v4, b), c, 0, 0, 0);
  }
};

// eight elements (one 16-byte load) as fp32
template <typename E> __device__ inline void elt_unpack8(const uint4 v, float* out) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    out[2 * j] = E::lo(w[j]);
    out[2 * j + 1] = E::hi(w[j]);
  }
}

// ---- OCP E4M3 (torch.float8_e4m3fn) codes of the fp8 KV cache (MXVL_KV_FP8, include/mxvl.h) ---------------------------------------
// gfx950's v_cvt_*_fp8 instructions are the OCP format (gfx942's were FNUZ: another bias, no negative zero).  A code times the
// tensor's power-of-two scale is exact in the model's 16-bit dtype, so code -> element needs no rounding: bf16 is the upper half of
// the fp32 bits, fp16 an exact narrowing.
// code = rne_e4m3(clamp(x, -448, 448)): the clamp is explicit (what the convert does above 448 depends on a mode bit); NaN stays NaN
__device__ inline uint32_t e4m3_encode(float x) {
  const float c = fminf(fmaxf(x, -448.0f), 448.0f);
  x = x != x ? x : c;
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x, x, 0, false) & 0xffu;
}
__device__ inline float e4m3_decode(uint32_t code) { return __builtin_amdgcn_cvt_f32_fp8((int)code, 0); }
// the four codes of a dword as fp32
__device__ inline void e4m3_unpack4(uint32_t w, float* out) {
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  out[0] = lo[0]; out[1] = lo[1]; out[2] = hi[0]; out[3] = hi[1];
}
// an E4M3 value (3 mantissa bits, |x| <= 448) as element bits: exact in both types
template <typename E> __device__ inline uint32_t e4m3_elt_bits(float x) {
  if constexpr (E::dtype == MXVL_BF16) return __builtin_bit_cast(uint32_t, x) >> 16;
  else return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x);
}
// two dwords of codes (eight elements) as the four packed dwords of a 16x16x32 MFMA operand
template <typename E> __device__ inline elt_u32x4 e4m3_unpack8_elt(uint32_t w0, uint32_t w1) {
  float f[8];
  e4m3_unpack4(w0, f);
  e4m3_unpack4(w1, f + 4);
  elt_u32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = e4m3_elt_bits<E>(f[2 * j]) | (e4m3_elt_bits<E>(f[2 * j + 1]) << 16);
  return r;
}
// 1 / s of a power-of-two scale s (a normal fp32): exact, no divide
__device__ inline float pow2_recip(float s) { return __builtin_bit_cast(float, 0x7f000000u - __builtin_bit_cast(uint32_t, s)); }

// ---- the format of the decode KV cache as a trait: what differs between the 16-bit and the E4M3 cache in decode_attn_kernel and ------
// decode_attn_beams_mfma_kernel (decode.hip).  LDS-DMA moves 16 bytes per lane, so a lane owns EPL elements of a cache row and
// D / EPL lanes share the row.
//   cache_t               one cache element: its size is the bytes per element
//   scaled                one power-of-two scale per tensor: K's rides on the (already scaled) query, V's on the final output, both
//                         exact, so what is summed are plain code values; without it (16-bit) no multiply is emitted at all
//   encode(x, 1/s)        the cache bits of a new element
//   value(bits, x)        the fp32 value those bits stand for: a new K / V enters this step's attention as the cache holds it, like
//                         every cached position (16-bit: x is already an element's value, and no instruction)
//   unpack(v, out)        the EPL elements of one 16-byte load as fp32
// and, for the beams kernel's LDS tile of 16 positions x D elements:
//   tile_key<D>(row)      the XOR key on the 16-byte unit index of a row (the swizzle is described at the kernel)
//   kraw_t, k_operand     what a lane reads from LDS for eight K elements, and the 16x16x32 A operand made of it
//   vraw_t, v_operand     what a lane reads from LDS for four V elements, and element i of the 16x16x16 A operand made of it
// The reads themselves stand in the kernel, per format: as trait functions they compiled the 16-bit kernel's LDS addresses
// differently.
template <typename KV, int D> __device__ __forceinline__ int kv_tile_off(int row, int unit) {
  return row * (D * (int)sizeof(typename KV::cache_t)) + ((unit ^ KV::template tile_key<D>(row)) << 4);
}
template <typename E> struct Kv16 {
  typedef uint16_t cache_t;
  static constexpr int EPL = 8;
  static constexpr bool scaled = false;
  __device__ static __forceinline__ uint32_t encode(float x, float) { return E::r(x); }
  __device__ static __forceinline__ float value(uint32_t, float x) { return x; }
  __device__ static __forceinline__ void unpack(const uint4 v, float* out) { elt_unpack8<E>(v, out); }
  template <int D> __device__ static __forceinline__ int tile_key(int row) {
    constexpr int UPR = D / 8;
    return UPR == 8 ? ((((row >> 1) & 1) << 2) | ((row >> 2) & 3)) : UPR == 16 ? (((row & 3) << 2) | ((row >> 2) & 3)) : (row & (UPR - 1));
  }
  typedef elt_u32x4 kraw_t;
  typedef elt_s16x4 vraw_t;
  __device__ static __forceinline__ elt_u32x4 k_operand(kraw_t k) { return k; }
  __device__ static __forceinline__ short v_operand(vraw_t v, int i) { return v[i]; }
};
// rows of D bytes: code = rne_e4m3(clamp(x / s)), widened with v_cvt_pk_f32_fp8, four codes per dword.  A code's value is exact in
// bf16 and fp16, so the MFMA operands are plain code values, made AFTER the LDS read.
template <typename E> struct KvE4m3 {
  typedef uint8_t cache_t;
  static constexpr int EPL = 16;
  static constexpr bool scaled = true;
  __device__ static __forceinline__ uint32_t encode(float x, float recip_scale) { return e4m3_encode(x * recip_scale); }
  __device__ static __forceinline__ float value(uint32_t code, float) { return e4m3_decode(code); }
  __device__ static __forceinline__ void unpack(const uint4 v, float* out) {
    e4m3_unpack4(v.x, out); e4m3_unpack4(v.y, out + 4); e4m3_unpack4(v.z, out + 8); e4m3_unpack4(v.w, out + 12);
  }
  template <int D> __device__ static __forceinline__ int tile_key(int row) { return D == 64 ? ((row >> 2) & 3) : ((row >> 1) & 7); }
  typedef uint2 kraw_t;
  struct vraw_t { uint32_t b[4]; };
  __device__ static __forceinline__ elt_u32x4 k_operand(kraw_t k) { return e4m3_unpack8_elt<E>(k.x, k.y); }
  __device__ static __forceinline__ short v_operand(vraw_t v, int i) { return (short)e4m3_elt_bits<E>(e4m3_decode(v.b[i])); }
};

// mxvl_dtype of a decode descriptor: 0 (what ABI <= 7 callers leave in the reserved field) means bf16
inline int decode_dtype(int32_t v) { return v == 0 ? MXVL_BF16 : v; }
// anything but bf16 / fp16 behind that default is refused (MXVL_ERR_DTYPE), not decoded as bf16
inline bool decode_dtype_ok(int32_t v) { return v == 0 || v == MXVL_BF16 || v == MXVL_F16; }
// the weight-format bits of mxvl_gemv_desc.dtype: at most one of them may be set
constexpr int kWeightFlags = MXVL_W_INT8 | MXVL_W_MXFP4 | MXVL_W_FP8 | MXVL_W_INT4;

}  // namespace mxvl
