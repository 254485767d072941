// mcaq_quant.h - pass 2 of the hook path (y = dequant(quant_b(x)) * m): the
// general, tile-aligned and reference-arithmetic kernels and their extern "C"
// launchers (include/mcaq_hip.h).  Included by mcaq_kernels.hip.
#pragma once

struct QuantArgs {
  mcaq_quant_scale s[MAXSEG];
  int nscales;
  int units_total;
  // tile-aligned path (mcaq_quant_tile_kernel): H = ht << sh, W = wt << sw;
  // reciprocals of the slice count, units per image and W for div_small
  int sh[MAXSEG], sw[MAXSEG];
  float rnsl[MAXSEG], rupi[MAXSEG], rw[MAXSEG];
};

// channels per unit (8 per wave).  Fixed: mcaq_quant_tile_kernel stores one
// [bits][channel] table entry per thread (bit width tid / 32, channel tid % 32)
// for 8 widths x QSLICE channels
constexpr int QSLICE = 32;
constexpr int QCW = QSLICE / 4;       // channels per wave
constexpr int QMAXBITS = 15;   // max entries per channel in the LDS table
constexpr int QMAXNT = 1024;   // max tiles per image whose m values are staged in LDS (more: read from L2)

// unit = 256 pixels x 32 channels of one image; lane l of every wave owns
// pixels 4l..4l+3 (16-byte accesses), wave w channels 8w..8w+7 of the slice,
// all eight rows loaded before any is computed.  Per-pixel tile bits and the
// soft-mask value are fetched once; per-(channel, bits) scale / zero-point
// come from an LDS table built by the workgroup (IEEE divisions, as
// QuantizationParameters computes them).
// 6 resident workgroups per CU (79 VGPRs, no spills): the prologue's early
// loads raised the unbounded kernel to 91 VGPRs / 5 workgroups; r02 A/B
// 29.7 vs 30.4-30.6 us back to back (profiles/r02_probes/ab_round2_late.txt);
// 7 spills 16 VGPRs
#ifndef MCAQ_QUANT_MINW
#define MCAQ_QUANT_MINW 6
#endif
#define MCAQ_QUANT_LB __launch_bounds__(256, MCAQ_QUANT_MINW)
// m(p) source of a pass-2 instantiation (compile time, so that no load sits
// behind a runtime branch: the compiler's wait counts then stay exact and the
// x rows stay in flight through the prologue -- with the loads behind
// branches it waited for every x row before the first barrier, r03)
enum : int { QM_NONE = 0, QM_MT_LDS = 1, QM_MT_L2 = 2, QM_PLANE = 3 };
// access policy of a general-kernel instantiation: element-wise rows, 16-byte
// rows with streaming stores of y, the same with nontemporal loads of x
enum : int { QP_ELEM = 0, QP_STREAM = 1, QP_NTLOAD = 2 };

// The three kernels spell their prologue out, each on its own.  Writing its
// steps once as inlined pieces (unit decode, table operands, m(tile) staging,
// bit width -> table row, the 5x5 Gaussian, the wave's vote) was tried: every
// piece but two changed the instruction order of the kernels using it, the
// fp32 m(tile) tile kernel then measured ~1 % slower, and the last two changed
// one reference kernel.  A fix to a prologue step goes into
// mcaq_quant_kernel, quant_tile_unit and quant_tile_unit_ref.

// pixel -> tile row / column: the reference's nearest source index
// floor(o * fp32(in / out)), clamped (exact for the o >> k and o >> 1 special
// cases of ATen's nearest_idx too: in / out is then a power of two), or the
// spatial_quantize contract o / tile, clamped; branch-free
__device__ __forceinline__ int q_tile_of(int o, int in, float sc, int compat_tile) {
  const int ns = imin_((int)floorf((float)o * sc), in - 1);
  const int ct = imin_(o / imax_(compat_tile, 1), in - 1);
  return compat_tile > 0 ? ct : ns;
}

// ---- the general kernel ------------------------------------------------------
// any map / tile-grid geometry (per-pixel tile lookup), up to QMAXBITS widths,
// m(p) from m(tile) values in LDS or L2 or from a given plane.  kBig: more
// than 256 table entries or staged m(tile) values.
template <int kP, int kM, bool kBig>
__global__ MCAQ_QUANT_LB void mcaq_quant_kernel(QuantArgs a) {
  constexpr bool kVec = kP != QP_ELEM, kNTL = kP == QP_NTLOAD, kNTS = kVec;
  __shared__ float4 qt[QSLICE * QMAXBITS];   // scale, zp, 1/scale
  __shared__ float mts[kM == QM_MT_LDS ? QMAXNT : 1];
  __shared__ float mq[256];
  __shared__ int qany[QSLICE];               // channel needs quant_dequant_any
  const int unit = blockIdx.x;
  int si = 0;
  while (si + 1 < a.nscales && unit >= a.s[si + 1].unit_begin) ++si;
  const mcaq_quant_scale& S = a.s[si];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int HW = S.H * S.W;
  const int upi = (HW + 255) / 256;
  const int nsl = (S.C + QSLICE - 1) / QSLICE;
  int lu = unit - S.unit_begin;
  const int slice = lu % nsl; lu /= nsl;
  const int chunk = lu % upi;
  const int b = lu / upi;
  const int c0 = slice * QSLICE;
  const int nc = imin_(QSLICE, S.C - c0);
  const int NB = S.nbits;
  const int NTq = S.ht * S.wt;
  const int ntab = nc * NB;
  // ---- 1. small operands, unconditional (clamped indices): this thread's
  // table entry's min / max, its m(tile) value, the lane's 4 tile bits (and
  // m(p) values when the plane is given)
  const int tc = imin_(tid / NB, nc - 1);
  const float tmn0 = S.xmin[c0 + tc], tmx = S.xmax[c0 + tc];
  const float tmn = S.neg_min ? -tmn0 : tmn0;
  float mtv = 0.0f;
  if (kM == QM_MT_LDS) mtv = S.mt[(size_t)b * NTq + imin_(tid, NTq - 1)];
  const int q0 = chunk * 256 + lane * 4;
  const float sch = (float)S.ht / (float)S.H, scw = (float)S.wt / (float)S.W;
  bool pv[4];
  float bv[4], mv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = imin_(q0 + k, HW - 1);
    pv[k] = q0 + k < HW;
    const int h = p / S.W, w = p - h * S.W;
    const int th = q_tile_of(h, S.ht, sch, S.compat_tile_h);
    const int tw = q_tile_of(w, S.wt, scw, S.compat_tile_w);
    bv[k] = S.bits[((size_t)b * S.ht + th) * S.wt + tw];
    mv[k] = kM == QM_PLANE ? S.m[(size_t)b * HW + p] : 1.0f;
  }
  // ---- 2. the x rows (8 x 16 B per lane), in flight through the prologue
  const int cw = wv * QCW;                 // first channel of this wave in the slice
  const int ncw = imin_(QCW, nc - cw);     // may be <= 0 for a short last slice
  const size_t rowbase = ((size_t)b * S.C + c0 + imax_(imin_(cw, nc - 1), 0)) * HW;
  const float* xb = S.x + rowbase;
  float* yb = S.y + rowbase;
  float v[QCW][4];
  const int qa = pv[0] ? q0 : 0;
#pragma unroll
  for (int c = 0; c < QCW; ++c) {
    const float* row = xb + (size_t)imin_(c, imax_(ncw - 1, 0)) * HW;
    if (kVec) {
      typedef float f4v __attribute__((ext_vector_type(4)));
      const f4v t = kNTL ? __builtin_nontemporal_load(reinterpret_cast<const f4v*>(row + qa))
                        : *reinterpret_cast<const f4v*>(row + qa);
      v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[c][k] = row[imin_(q0 + k, HW - 1)];
    }
  }
  // ---- 3. scale / zero-point table and staged m values (no global loads
  // behind a branch on the common path; > 256 entries only in kBig builds)
  {
    // every thread computes an entry (tid >= ntab: an unused slot of the
    // 480-entry table), so the min / max loads have an unconditional use and
    // are not sunk into a branch behind the x rows
    const int kq = imin_(tid - tc * NB, QMAXBITS - 1);
    const QParam q = qparam(tmn, tmx, S.bits_lo + kq);
    qt[tid] = make_float4(q.scale, q.zp, q.rs, 0.0f);
    if (kq == 0) qany[tc] = (!S.stats_cover_x || stats_need_any(tmn, tmx)) ? 1 : 0;
  }
  if (kBig) {
    for (int i = tid + 256; i < ntab; i += 256) {   // > 256 entries: continuous bit ranges
      const int c = i / NB, k = i - (i / NB) * NB;
      const float mn = S.neg_min ? -S.xmin[c0 + c] : S.xmin[c0 + c];
      const QParam q = qparam(mn, S.xmax[c0 + c], S.bits_lo + k);
      qt[i] = make_float4(q.scale, q.zp, q.rs, 0.0f);
      if (k == 0) qany[c] = (!S.stats_cover_x || stats_need_any(mn, S.xmax[c0 + c])) ? 1 : 0;
    }
  }
  if (kM == QM_MT_LDS) {
    if (tid < NTq) mts[tid] = mtv;
    if (kBig)
      for (int i = tid + 256; i < NTq; i += 256) mts[i] = S.mt[(size_t)b * NTq + i];
  }
  int kb[4];
  float qlo[4], qhi[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    kb[k] = imin_(imax_((int)rintf(bv[k]), S.bits_lo), S.bits_lo + NB - 1) - S.bits_lo;
    const int bb = S.bits_lo + kb[k];
    qlo[k] = (float)(-(1 << (bb - 1)));
    qhi[k] = (float)((1 << (bb - 1)) - 1);
  }
  __syncthreads();   // qt, mts ready
  if (kM == QM_MT_LDS || kM == QM_MT_L2) {
    // m(p) = 5x5 Gaussian (replicate pad) of the nearest-upsampled tile values,
    // taps row-major from 0 - the m plane LearnedSoftMask produces
    // (quantization.py:235-238), generated here instead of read from HBM.
    // Wave w computes pixel w of every lane's quad; the quads meet in LDS.
    const float* mtab = kM == QM_MT_LDS ? mts : S.mt + (size_t)b * NTq;
    {
      const int p = imin_(q0 + wv, HW - 1);
      const int h = p / S.W, w = p - h * S.W;
      int cs[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) cs[j] = q_tile_of(imin_(imax_(w + j - 2, 0), S.W - 1), S.wt, scw, 0);
      float acc = 0.0f;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int rb = q_tile_of(imin_(imax_(h + i - 2, 0), S.H - 1), S.ht, sch, 0) * S.wt;
#pragma unroll
        for (int j = 0; j < 5; ++j) acc = fmaf(bits_as_float(k_smooth5_bits[i * 5 + j]), mtab[rb + cs[j]], acc);
      }
      mq[lane * 4 + wv] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) mv[k] = mq[lane * 4 + k];
  }
  if (ncw <= 0) return;
  // one wave-uniform choice for the wave's channels: the short arithmetic
  // unless a channel's statistics do not cover x or are not finite
  int anyc = 0;
#pragma unroll
  for (int c = 0; c < QCW; ++c) anyc |= c < ncw ? qany[cw + c] : 0;
  const bool any_x = __builtin_amdgcn_readfirstlane(anyc) != 0;
#pragma unroll
  for (int c = 0; c < QCW; ++c) {
    if (c >= ncw) break;
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 sz = qt[(cw + c) * NB + kb[k]];
      QParam q;
      q.scale = sz.x; q.zp = sz.y; q.rs = sz.z; q.qmin = qlo[k]; q.qmax = qhi[k];
      float d = any_x ? quant_dequant_any(v[c][k], q) : quant_dequant(v[c][k], q);
      if (kM != QM_NONE) d = d * mv[k];
      o[k] = d;
    }
    float* orow = yb + (size_t)c * HW;
    if (kVec) {
      if (pv[0]) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v ov = {o[0], o[1], o[2], o[3]};
        // y is written once and not re-read by this step: streaming store
        if (kNTS) __builtin_nontemporal_store(ov, reinterpret_cast<f4v*>(orow + q0));
        else *reinterpret_cast<f4v*>(orow + q0) = ov;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (pv[k]) orow[q0 + k] = o[k];
    }
  }
}

// ---- the tile-aligned family -------------------------------------------------
// When every scale's map is a power-of-two multiple of its tile grid
// (H = ht << sh, W = wt << sw, sw >= 2 - every hook scale), a lane's 4
// consecutive pixels lie in ONE tile: one bit width, so one (scale, zp,
// 1/scale) table entry per channel serves all 4, read from a [bits][channel]
// LDS table at an immediate offset, and the quantizer runs on pixel pairs with
// packed fp32 instructions (v_pk_mul / v_pk_fma / v_pk_add, each an IEEE fp32
// operation per component: the values are those of quant_dequant).  Pixel ->
// tile and m(p)'s source rows / columns are shifts; no integer division
// anywhere (the general kernel spent
// ~2/3 of its ~1,070 VALU instructions per wave on index arithmetic and its
// integer divisions: rocprofv3 SQ_INSTS_VALU, profiles/r04_sq/).  Soft mask:
// none or m(tile) values (QM_NONE / QM_MT_LDS); at most 8 bit widths.  y is
// fp32, stored with streaming stores.

template <bool kNTL, bool kNTS, int kM, typename T, typename TO>
__device__ __forceinline__ void quant_tile_unit(const QuantArgs& a, const int unit, float4* qt, float* mts, float4* mq4,
                                                int* qany) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  int si = 0;
  while (si + 1 < a.nscales && unit >= a.s[si + 1].unit_begin) ++si;
  const mcaq_quant_scale& S = a.s[si];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int H = S.H, W = S.W, HW = H * W;
  const int sh = a.sh[si], sw = a.sw[si];
  const float rnsl = a.rnsl[si], rupi = a.rupi[si], rw = a.rw[si];
  const int nsl = (S.C + QSLICE - 1) / QSLICE, upi = (HW + 255) >> 8;
  const int lu = unit - S.unit_begin;
  const int q1 = div_small(lu, nsl, rnsl);
  const int slice = lu - q1 * nsl;
  const int b = div_small(q1, upi, rupi);
  const int chunk = q1 - b * upi;
  const int c0 = slice * QSLICE;
  const int nc = imin_(QSLICE, S.C - c0);
  const int NB = S.nbits;
  const int NTq = S.ht * S.wt;
  // ---- 1. small operands: this thread's table entry (bit width tid / 32,
  // channel tid % 32), its m(tile) value, the lane's tile bits (one load: its
  // 4 pixels share the tile)
  const int tc = imin_(tid & (QSLICE - 1), nc - 1);
  const float tmn0 = S.xmin[c0 + tc], tmx = S.xmax[c0 + tc];
  const float tmn = S.neg_min ? -tmn0 : tmn0;
  float mtv = 0.0f;
  if (kM == QM_MT_LDS) mtv = S.mt[(size_t)b * NTq + imin_(tid, NTq - 1)];
  const int q0 = chunk * 256 + lane * 4;
  const bool pv = q0 < HW;                     // HW % 4 == 0: all 4 pixels in or out
  const int qa = pv ? q0 : 0;
  const int h0 = div_small(qa, W, rw), w0 = qa - h0 * W;
  const float bv = S.bits[((size_t)b * S.ht + (h0 >> sh)) * S.wt + (w0 >> sw)];
  // ---- 2. the x rows (8 x 16 B per lane), in flight through the prologue
  const int cw = wv * QCW;
  const int ncw = imin_(QCW, nc - cw);
  const size_t rowbase = ((size_t)b * S.C + c0 + imax_(imin_(cw, nc - 1), 0)) * HW;
  const T* xb = reinterpret_cast<const T*>(S.x) + rowbase;
  TO* yb = reinterpret_cast<TO*>(S.y) + rowbase;
  typedef float f4v __attribute__((ext_vector_type(4)));
  f4v v[QCW];
#pragma unroll
  for (int c = 0; c < QCW; ++c) v[c] = ElemIO<T>::template ld4<kNTL>(xb + (size_t)imin_(c, imax_(ncw - 1, 0)) * HW + qa);
  // ---- 3. the table (IEEE divisions of QuantizationParameters), staged m(tile)
  {
    const int kq = imin_(tid >> 5, NB - 1);     // every thread stores an entry (unused rows harmless)
    const QParam q = qparam(tmn, tmx, S.bits_lo + kq);
    qt[tid] = make_float4(q.scale, q.zp, q.rs, 0.0f);
    if (tid < QSLICE) qany[tid] = (!S.stats_cover_x || stats_need_any(tmn, tmx)) ? 1 : 0;
  }
  if (kM == QM_MT_LDS) {
    if (tid < NTq) mts[tid] = mtv;
    for (int i = tid + 256; i < NTq; i += 256) mts[i] = S.mt[(size_t)b * NTq + i];
  }
  const int kb = imin_(imax_((int)rintf(bv), S.bits_lo), S.bits_lo + NB - 1) - S.bits_lo;
  const int hb = 1 << (S.bits_lo + kb - 1);
  const float qlo = (float)(-hb), qhi = (float)(hb - 1);
  __syncthreads();   // qt, mts ready
  // ---- 4. m(p) = 5x5 Gaussian (replicate pad) of the nearest-upsampled tile
  // values, taps row-major from 0 (quantization.py:235-238); wave w computes
  // pixel w of every lane's quad
  f2 m01 = {1.0f, 1.0f}, m23 = {1.0f, 1.0f};
  if (kM == QM_MT_LDS) {
    const int w = w0 + wv;
    int cs[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) cs[j] = imin_(imax_(w + j - 2, 0), W - 1) >> sw;
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int rb = (imin_(imax_(h0 + i - 2, 0), H - 1) >> sh) * S.wt;
#pragma unroll
      for (int j = 0; j < 5; ++j) acc = fmaf(bits_as_float(k_smooth5_bits[i * 5 + j]), mts[rb + cs[j]], acc);
    }
    reinterpret_cast<float*>(mq4)[lane * 4 + wv] = acc;
    __syncthreads();
    const float4 mm = mq4[lane];
    m01 = f2{mm.x, mm.y};
    m23 = f2{mm.z, mm.w};
  }
  if (ncw <= 0) return;
  int anyc = 0;
#pragma unroll
  for (int c = 0; c < QCW; ++c) anyc |= c < ncw ? qany[cw + c] : 0;
  const bool any_x = __builtin_amdgcn_readfirstlane(anyc) != 0;
  const float4* qrow = qt + kb * QSLICE + cw;   // the lane's entries: immediate offsets c * 16
#pragma unroll
  for (int c = 0; c < QCW; ++c) {
    if (c >= ncw) break;
    const float4 e = qrow[c];
    f4v o;
    if (!any_x) {
      // quant_dequant (mcaq_math.h) on pixel pairs: x / s by the reciprocal
      // and one FMA correction, + zp, round half to even, clamp, - zp, * s, * m
      const f2 x01 = f2{v[c].x, v[c].y}, x23 = f2{v[c].z, v[c].w};
      const f2 s2 = f2{e.x, e.x}, r2 = f2{e.z, e.z};
      const f2 p01 = x01 * e.z, p23 = x23 * e.z;
      const f2 d01 = __builtin_elementwise_fma(__builtin_elementwise_fma(-p01, s2, x01), r2, p01);
      const f2 d23 = __builtin_elementwise_fma(__builtin_elementwise_fma(-p23, s2, x23), r2, p23);
      f2 t01 = d01 + e.y, t23 = d23 + e.y;
      t01.x = __builtin_amdgcn_fmed3f(rintf(t01.x), qlo, qhi);
      t01.y = __builtin_amdgcn_fmed3f(rintf(t01.y), qlo, qhi);
      t23.x = __builtin_amdgcn_fmed3f(rintf(t23.x), qlo, qhi);
      t23.y = __builtin_amdgcn_fmed3f(rintf(t23.y), qlo, qhi);
      f2 y01 = (t01 - e.y) * e.x, y23 = (t23 - e.y) * e.x;
      if (kM != QM_NONE) { y01 = y01 * m01; y23 = y23 * m23; }
      o = f4v{y01.x, y01.y, y23.x, y23.y};
    } else {
      QParam q;
      q.scale = e.x; q.zp = e.y; q.rs = e.z; q.qmin = qlo; q.qmax = qhi;
      o = f4v{quant_dequant_any(v[c].x, q), quant_dequant_any(v[c].y, q), quant_dequant_any(v[c].z, q),
              quant_dequant_any(v[c].w, q)};
      if (kM != QM_NONE) o = o * f4v{m01.x, m01.y, m23.x, m23.y};
    }
    if (pv) ElemIO<TO>::template st4<kNTS>(yb + (size_t)c * HW + q0, o);
  }
}

template <bool kNTL, int kM, typename T = float>
__global__ MCAQ_QUANT_LB void mcaq_quant_tile_kernel(QuantArgs a) {
  __shared__ float4 qt[8 * QSLICE];           // [kb][c]: scale, zp, 1/scale
  __shared__ float mts[kM == QM_MT_LDS ? QMAXNT : 1];
  __shared__ float4 mq4[64];                  // m(p) of each lane's 4 pixels
  __shared__ int qany[QSLICE];
  quant_tile_unit<kNTL, true, kM, T, float>(a, (int)blockIdx.x, qt, mts, mq4, qany);
}

// ---------------------------------------------------------------------------
// pass 2 in the reference's half arithmetic (mcaq_quant_scale.arith =
// MCAQ_ARITH_REFERENCE): an fp16 / bf16 map at inference with the batch's own
// statistics.  The reference runs QuantizationParameters and quantize_tensor
// on the half tensors themselves (quantization.py:41-66, 409-434, 561-602), so
// every elementwise result is rounded to the map's dtype, and sums x_q * mask
// over the widths present in the bit map in fp32 (:729-738).  With r() =
// round-to-nearest-even to the map's dtype:
//   rng = max(r(max - min), r(1e-8))        s = r(rng / (qmax - qmin))
//   zp  = clamp(r(qmin - r(min / s)), qmin, qmax)
//   t   = r(r(x / s) + zp)
//   xq  = r(r(clamp(rint(t), qmin, qmax) - zp) * s)        y = (0 + xq) * m
// Each r(a op b) of two half values equals the native half operation (fp32
// carries 24 >= 2 p + 2 bits: the double rounding is innocuous), so fp16 runs
// its chain in v_*_f16 and bf16 in fp32 + one conversion per operation.  x / s
// is div_by (mcaq_math.h): the correctly rounded fp32 quotient, whose rounding
// to half is the half quotient.
// Same unit geometry, loads and stores as quant_tile_unit.  The table carries
// a flag per (width, channel) entry: set when the short chain is not provably
// the literal one (s zero / non-finite / outside 1e-30..1e30, a NaN zero point,
// |x| / s beyond 1e12, or (qmax - qmin) * s overflowing the dtype).  A wave
// with a flagged entry among its 8 channels (at any width) takes the literal
// chain: IEEE divisions, NaN-propagating clamps, and the reference's sum over
// every width present in the scale's bit map - x_q * 0 of a non-finite x_q at
// another width makes y NaN there.
// ---------------------------------------------------------------------------
template <typename T> struct RefHalf;
template <> struct RefHalf<_Float16> {
  static constexpr int DT = MCAQ_DTYPE_F16;
  static __device__ __forceinline__ float r(float v) { return (float)(_Float16)v; }
  // r(r(med3(rint(r(r(d) + zp)), qlo, qhi) - zp) * s) for finite operands
  static __device__ __forceinline__ float chain(float d, float s, float zp, float qlo, float qhi) {
    const _Float16 zh = (_Float16)zp, sh = (_Float16)s;
    const _Float16 dh = (_Float16)d;
    const _Float16 t = dh + zh;
    const _Float16 q = __builtin_amdgcn_fmed3h(__builtin_rintf16(t), (_Float16)qlo, (_Float16)qhi);
    const _Float16 u = q - zh;
    const _Float16 xq = u * sh;
    return (float)xq;
  }
};
template <> struct RefHalf<Bf16> {
  static constexpr int DT = MCAQ_DTYPE_BF16;
  static __device__ __forceinline__ float r(float v) { return round_bf16(v); }
  static __device__ __forceinline__ float rf(float v) {   // finite v
    const uint32_t u = __float_as_uint(v);
    return __uint_as_float((u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u);
  }
  static __device__ __forceinline__ float chain(float d, float s, float zp, float qlo, float qhi) {
    const float t = rf(rf(d) + zp);
    const float q = __builtin_amdgcn_fmed3f(rintf(t), qlo, qhi);
    return rf(rf(q - zp) * s);
  }
};

// one [width][channel] table entry: (s, zp, RN(1 / s), flag)
template <typename T>
__device__ __forceinline__ float4 ref_qentry(float mn, float mx, int bits) {
  typedef RefHalf<T> R;
  const float qmin = (float)(-(1 << (bits - 1))), qmax = (float)((1 << (bits - 1)) - 1);
  const float rng = fmaxp(R::r(mx - mn), R::r(1e-8f));          // torch.clamp(min=): NaN stays
  const float s = R::r(rng / (qmax - qmin));
  const float zp = clamp_nan(R::r(qmin - R::r(mn / s)), qmin, qmax);
  const float big = fmaxf(fabsf(mn), fabsf(mx)) / s;
  const bool safe = mn == mn && mx == mx && s >= 1e-30f && s <= 1e30f && big < 1e12f && zp == zp &&
                    fabsf(R::r((qmax - qmin) * s)) <= 3.40282347e38f;
  return make_float4(s, zp, 1.0f / s, safe ? 0.0f : 1.0f);
}

// the literal chain of one element at one width (any operand)
template <typename T>
__device__ __forceinline__ float ref_xq_any(float x, float4 e, float qlo, float qhi) {
  typedef RefHalf<T> R;
  const float t = R::r(R::r(x / e.x) + e.y);
  const float q = clamp_nan(rintf(t), qlo, qhi);
  return R::r(R::r(q - e.y) * e.x);
}

template <int kM, typename T>
__device__ __forceinline__ void quant_tile_unit_ref(const QuantArgs& a, const int unit, float4* qt, float* mts,
                                                    float4* mq4, int* qanyw) {
  typedef RefHalf<T> R;
  typedef float f4v __attribute__((ext_vector_type(4)));
  int si = 0;
  while (si + 1 < a.nscales && unit >= a.s[si + 1].unit_begin) ++si;
  const mcaq_quant_scale& S = a.s[si];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int H = S.H, W = S.W, HW = H * W;
  const int sh = a.sh[si], sw = a.sw[si];
  const int nsl = (S.C + QSLICE - 1) / QSLICE, upi = (HW + 255) >> 8;
  const int lu = unit - S.unit_begin;
  const int q1 = div_small(lu, nsl, a.rnsl[si]);
  const int slice = lu - q1 * nsl;
  const int b = div_small(q1, upi, a.rupi[si]);
  const int chunk = q1 - b * upi;
  const int c0 = slice * QSLICE;
  const int nc = imin_(QSLICE, S.C - c0);
  const int NB = S.nbits;
  const int NTq = S.ht * S.wt;
  // ---- 1. small operands (as quant_tile_unit)
  const int tc = imin_(tid & (QSLICE - 1), nc - 1);
  const float tmn0 = S.xmin[c0 + tc], tmx = S.xmax[c0 + tc];
  const float tmn = S.neg_min ? -tmn0 : tmn0;
  float mtv = 0.0f;
  if (kM == QM_MT_LDS) mtv = S.mt[(size_t)b * NTq + imin_(tid, NTq - 1)];
  const int q0 = chunk * 256 + lane * 4;
  const bool pv = q0 < HW;
  const int qa = pv ? q0 : 0;
  const int h0 = div_small(qa, W, a.rw[si]), w0 = qa - h0 * W;
  const float bv = S.bits[((size_t)b * S.ht + (h0 >> sh)) * S.wt + (w0 >> sw)];
  // ---- 2. the x rows (8 x 8 B per lane), widened exactly
  const int cw = wv * QCW;
  const int ncw = imin_(QCW, nc - cw);
  const size_t rowbase = ((size_t)b * S.C + c0 + imax_(imin_(cw, nc - 1), 0)) * HW;
  const T* xb = reinterpret_cast<const T*>(S.x) + rowbase;
  float* yb = S.y + rowbase;
  f4v v[QCW];
#pragma unroll
  for (int c = 0; c < QCW; ++c) v[c] = ElemIO<T>::template ld4<true>(xb + (size_t)imin_(c, imax_(ncw - 1, 0)) * HW + qa);
  // ---- 3. the table in the map's arithmetic, the flags, staged m(tile)
  {
    const int kq = imin_(tid >> 5, NB - 1);
    const float4 e = ref_qentry<T>(tmn, tmx, S.bits_lo + kq);
    qt[tid] = e;
    int f = e.w != 0.0f ? 1 : 0;
    f |= __shfl_xor(f, 32, 64);                 // the wave's two width rows
    if (lane < QSLICE) qanyw[wv * QSLICE + lane] = f;
  }
  if (kM == QM_MT_LDS) {
    if (tid < NTq) mts[tid] = mtv;
    for (int i = tid + 256; i < NTq; i += 256) mts[i] = S.mt[(size_t)b * NTq + i];
  }
  const int kb = imin_(imax_((int)rintf(bv), S.bits_lo), S.bits_lo + NB - 1) - S.bits_lo;
  const int hb = 1 << (S.bits_lo + kb - 1);
  const float qlo = (float)(-hb), qhi = (float)(hb - 1);
  __syncthreads();   // qt, qanyw, mts ready
  // ---- 4. m(p) (as quant_tile_unit)
  f4v m4 = {1.0f, 1.0f, 1.0f, 1.0f};
  if (kM == QM_MT_LDS) {
    const int w = w0 + wv;
    int cs[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) cs[j] = imin_(imax_(w + j - 2, 0), W - 1) >> sw;
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int rb = (imin_(imax_(h0 + i - 2, 0), H - 1) >> sh) * S.wt;
#pragma unroll
      for (int j = 0; j < 5; ++j) acc = fmaf(bits_as_float(k_smooth5_bits[i * 5 + j]), mts[rb + cs[j]], acc);
    }
    reinterpret_cast<float*>(mq4)[lane * 4 + wv] = acc;
    __syncthreads();
    const float4 mm = mq4[lane];
    m4 = f4v{mm.x, mm.y, mm.z, mm.w};
  }
  if (ncw <= 0) return;
  // a flagged (width, channel) entry among this wave's channels: every width
  // row of the table, since another width's x_q can reach y through x_q * 0
  int fl = 0;
  {
    const int rl = lane & 31;
    if ((rl & 7) < ncw) fl = qanyw[(rl >> 3) * QSLICE + cw + (rl & 7)];
  }
  const bool any_x = __builtin_amdgcn_ballot_w64(fl != 0) != 0;
  const float4* qrow = qt + kb * QSLICE + cw;
  if (!any_x) {
#pragma unroll
    for (int c = 0; c < QCW; ++c) {
      if (c >= ncw) break;
      const float4 e = qrow[c];
      f4v o;
      o.x = R::chain(div_by(v[c].x, e.x, e.z), e.x, e.y, qlo, qhi) + 0.0f;
      o.y = R::chain(div_by(v[c].y, e.x, e.z), e.x, e.y, qlo, qhi) + 0.0f;
      o.z = R::chain(div_by(v[c].z, e.x, e.z), e.x, e.y, qlo, qhi) + 0.0f;
      o.w = R::chain(div_by(v[c].w, e.x, e.z), e.x, e.y, qlo, qhi) + 0.0f;
      if (kM != QM_NONE) o = o * m4;
      if (pv) ElemIO<float>::template st4<true>(yb + (size_t)c * HW + q0, o);
    }
    return;
  }
  // the widths present in the scale's bit map (torch.unique over all B images)
  unsigned pm = 0;
  for (int j = lane; j < S.B * NTq; j += 64)
    pm |= 1u << (imin_(imax_((int)rintf(S.bits[j]), S.bits_lo), S.bits_lo + NB - 1) - S.bits_lo);
  for (int o = 32; o > 0; o >>= 1) pm |= (unsigned)__shfl_xor((int)pm, o, 64);
#pragma unroll 1
  for (int c = 0; c < ncw; ++c) {
    float xs[4] = {v[0].x, v[0].y, v[0].z, v[0].w};
#pragma unroll
    for (int cc = 1; cc < QCW; ++cc)
      if (cc == c) { xs[0] = v[cc].x; xs[1] = v[cc].y; xs[2] = v[cc].z; xs[3] = v[cc].w; }
    float own[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool bad[4] = {false, false, false, false};
#pragma unroll 1
    for (int w = 0; w < NB; ++w) {
      if (!((pm >> w) & 1u)) continue;
      const float4 e = qt[w * QSLICE + cw + c];
      const int hw = 1 << (S.bits_lo + w - 1);
      const float wlo = (float)(-hw), whi = (float)(hw - 1);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xq = ref_xq_any<T>(xs[k], e, wlo, whi);
        if (w == kb) own[k] = xq;
        else bad[k] = bad[k] || !(fabsf(xq) <= 3.40282347e38f);
      }
    }
    f4v o;
    o.x = bad[0] ? __builtin_nanf("") : own[0] + 0.0f;
    o.y = bad[1] ? __builtin_nanf("") : own[1] + 0.0f;
    o.z = bad[2] ? __builtin_nanf("") : own[2] + 0.0f;
    o.w = bad[3] ? __builtin_nanf("") : own[3] + 0.0f;
    if (kM != QM_NONE) o = o * m4;
    if (pv) ElemIO<float>::template st4<true>(yb + (size_t)c * HW + q0, o);
  }
}

template <int kM, typename T>
__global__ MCAQ_QUANT_LB void mcaq_quant_tile_ref_kernel(QuantArgs a) {
  __shared__ float4 qt[8 * QSLICE];           // [kb][c]: s, zp, 1/s, flag
  __shared__ float mts[kM == QM_MT_LDS ? QMAXNT : 1];
  __shared__ float4 mq4[64];
  __shared__ int qanyw[4 * QSLICE];           // [wave][c]: a flagged entry in the wave's width rows
  quant_tile_unit_ref<kM, T>(a, (int)blockIdx.x, qt, mts, mq4, qanyw);
}

// ---------------------------------------------------------------------------
// host: validate (quant_args) -> choose (quant_plan) -> launch (quant_launch)
// ---------------------------------------------------------------------------
// the arguments of a pass-2 launch; returns 0 or a hipError_t
static int quant_args(const mcaq_quant_scale* scales, int nscales, QuantArgs& a) {
  if (nscales < 1 || nscales > MAXSEG) return (int)hipErrorInvalidValue;
  int units = 0;
  for (int i = 0; i < nscales; ++i) {
    const mcaq_quant_scale& q = scales[i];
    a.s[i] = q;
    a.s[i].unit_begin = units;
    const int HW = q.H * q.W;
    if (q.nbits < 1 || q.nbits > QMAXBITS || q.bits_lo < 1 || q.bits_lo + q.nbits - 1 > 16 || HW < 1 || q.C < 1 ||
        q.ht < 1 || q.wt < 1 || !q.x || !q.y || !q.bits || !q.xmin || !q.xmax || q.dtype != scales[0].dtype ||
        q.dtype < MCAQ_DTYPE_F32 || q.dtype > MCAQ_DTYPE_BF16 || q.ydtype != MCAQ_DTYPE_F32 ||
        q.arith < MCAQ_ARITH_FP32 || q.arith > MCAQ_ARITH_REFERENCE)
      return (int)hipErrorInvalidValue;
    // the reference's half arithmetic: a half map quantized with its own batch
    // statistics at widths <= 8 bits (exact in fp16 and bf16), one mode per launch
    if (q.arith != scales[0].arith) return (int)hipErrorNotSupported;
    if (q.arith == MCAQ_ARITH_REFERENCE &&
        (q.dtype == MCAQ_DTYPE_F32 || !q.stats_cover_x || q.m || q.bits_lo + q.nbits - 1 > 8))
      return (int)hipErrorNotSupported;
    // the tile-aligned family's shifts (H <= ht << sh, W <= wt << sw) and reciprocals
    int sh = 0, sw = 0;
    while ((q.ht << sh) < q.H) ++sh;
    while ((q.wt << sw) < q.W) ++sw;
    a.sh[i] = sh; a.sw[i] = sw;
    a.rnsl[i] = 1.0f / (float)((q.C + QSLICE - 1) / QSLICE);
    a.rupi[i] = 1.0f / (float)((HW + 255) / 256);
    a.rw[i] = 1.0f / (float)q.W;
    units += q.B * ((HW + 255) / 256) * ((q.C + QSLICE - 1) / QSLICE);
  }
  a.nscales = nscales;
  a.units_total = units;
  return 0;
}

// which kernel a validated launch takes
enum : int { QF_GENERAL, QF_TILE, QF_REF, QF_PER_SCALE, QF_UNSUPPORTED };
struct QuantPlan {
  int family, kind, dtype;   // kind: QM_*, one m(p) source for every scale of a launch
  bool big, vec, ntl;        // > 256 table entries or staged tiles; 16-byte rows; nontemporal loads of x
};

static QuantPlan quant_plan(const QuantArgs& a) {
  QuantPlan p{QF_GENERAL, -1, a.s[0].dtype, false, true, false};
  bool tile = true;
  size_t xbytes = 0;
  for (int i = 0; i < a.nscales; ++i) {
    const mcaq_quant_scale& q = a.s[i];
    const int NT = q.ht * q.wt;
    // m(p) source (the hook always passes m(tile) values or nothing; the
    // reference op a plane or nothing); mixed kinds: one launch per scale
    const int k = q.mt ? (NT <= QMAXNT ? QM_MT_LDS : QM_MT_L2) : (q.m ? QM_PLANE : QM_NONE);
    if (p.kind >= 0 && k != p.kind) { p.family = QF_PER_SCALE; return p; }
    p.kind = k;
    p.big = p.big || imin_(QSLICE, q.C) * q.nbits > 256 || (k == QM_MT_LDS && NT > 256);
    // 16-byte rows: HW % 4 == 0 and 16-byte aligned x / y bases (a contiguous
    // view may start at any float offset), else the element-wise kernel
    p.vec = p.vec && ((q.H * q.W) & 3) == 0 && (((uintptr_t)q.x | (uintptr_t)q.y) & 15) == 0;
    xbytes += (size_t)q.B * q.C * q.H * q.W * (q.dtype ? 2 : sizeof(float));
    // tile-aligned: the map a power-of-two multiple of the tile grid (tiles
    // >= 4 pixels wide), <= 8 bit widths, no compat indexing
    tile = tile && (q.ht << a.sh[i]) == q.H && (q.wt << a.sw[i]) == q.W && a.sw[i] >= 2 && q.nbits <= 8 &&
           q.compat_tile_h <= 0 && q.compat_tile_w <= 0 && NT <= QMAXNT;
  }
  tile = tile && p.vec && (p.kind == QM_NONE || p.kind == QM_MT_LDS);
  // nontemporal policy (measured): streaming stores of y always;
  // nontemporal loads of x only when the launch reads > 256 MB of it (config 3:
  // nothing of x survives in L2/MALL anyway), and in every half-map kernel
  p.ntl = p.dtype != MCAQ_DTYPE_F32 || xbytes > ((size_t)256 << 20);
  if (p.dtype != MCAQ_DTYPE_F32)   // fp16 / bf16 maps: the tile-aligned family only
    p.family = !tile ? QF_UNSUPPORTED : (a.s[0].arith == MCAQ_ARITH_REFERENCE ? QF_REF : QF_TILE);
  else if (tile)
    p.family = QF_TILE;
  return p;
}

typedef void (*QuantKernel)(QuantArgs);
// general [policy][kind][big]; QM_MT_L2 has the big build only
template <int kP>
struct QuantGeneral { static const QuantKernel k[4][2]; };
template <int kP>
const QuantKernel QuantGeneral<kP>::k[4][2] = {
    {mcaq_quant_kernel<kP, QM_NONE, false>, mcaq_quant_kernel<kP, QM_NONE, true>},
    {mcaq_quant_kernel<kP, QM_MT_LDS, false>, mcaq_quant_kernel<kP, QM_MT_LDS, true>},
    {mcaq_quant_kernel<kP, QM_MT_L2, true>, mcaq_quant_kernel<kP, QM_MT_L2, true>},
    {mcaq_quant_kernel<kP, QM_PLANE, false>, mcaq_quant_kernel<kP, QM_PLANE, true>}};
static const QuantKernel (*const k_quant_general[3])[2] = {QuantGeneral<QP_ELEM>::k, QuantGeneral<QP_STREAM>::k,
                                                           QuantGeneral<QP_NTLOAD>::k};
// tile [fp32, fp32 with nontemporal loads, fp16, bf16][none, m(tile)]
static const QuantKernel k_quant_tile[4][2] = {
    {mcaq_quant_tile_kernel<false, QM_NONE>, mcaq_quant_tile_kernel<false, QM_MT_LDS>},
    {mcaq_quant_tile_kernel<true, QM_NONE>, mcaq_quant_tile_kernel<true, QM_MT_LDS>},
    {mcaq_quant_tile_kernel<true, QM_NONE, _Float16>, mcaq_quant_tile_kernel<true, QM_MT_LDS, _Float16>},
    {mcaq_quant_tile_kernel<true, QM_NONE, Bf16>, mcaq_quant_tile_kernel<true, QM_MT_LDS, Bf16>}};
// reference arithmetic [fp16, bf16][none, m(tile)]
static const QuantKernel k_quant_ref[2][2] = {
    {mcaq_quant_tile_ref_kernel<QM_NONE, _Float16>, mcaq_quant_tile_ref_kernel<QM_MT_LDS, _Float16>},
    {mcaq_quant_tile_ref_kernel<QM_NONE, Bf16>, mcaq_quant_tile_ref_kernel<QM_MT_LDS, Bf16>}};

static int quant_launch(const QuantArgs& a, const QuantPlan& p, hipStream_t stream) {
  QuantKernel k;
  const int mt = p.kind == QM_NONE ? 0 : 1;
  switch (p.family) {
    case QF_GENERAL: k = k_quant_general[!p.vec ? QP_ELEM : (p.ntl ? QP_NTLOAD : QP_STREAM)][p.kind][p.big ? 1 : 0]; break;
    case QF_TILE: k = k_quant_tile[p.dtype == MCAQ_DTYPE_F32 ? (p.ntl ? 1 : 0) : p.dtype + 1][mt]; break;
    case QF_REF: k = k_quant_ref[p.dtype - MCAQ_DTYPE_F16][mt]; break;
    default: return (int)hipErrorNotSupported;
  }
  launch_k(k, dim3(a.units_total), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}

extern "C" {

int mcaq_quant(const mcaq_quant_scale* scales, int nscales, hipStream_t stream) {
  QuantArgs a;
  int e = quant_args(scales, nscales, a);
  if (e) return e;
  const QuantPlan p = quant_plan(a);
  if (p.family != QF_PER_SCALE) return quant_launch(a, p, stream);
  for (int j = 0; j < nscales; ++j) {
    e = quant_args(&scales[j], 1, a);
    if (!e) e = quant_launch(a, quant_plan(a), stream);
    if (e) return e;
  }
  return 0;
}

int mcaq_launch_spatial_quantization(const float* input, const float* bit_map, const float* min_vals,
                                     const float* max_vals, const float* mask, float* output, int N, int C,
                                     int H, int W, int tile_h, int tile_w, int n_tiles_h, int n_tiles_w,
                                     hipStream_t stream) {
  if (N < 1 || C < 1 || H < 1 || W < 1 || tile_h < 1 || tile_w < 1 || n_tiles_h < 1 || n_tiles_w < 1)
    return (int)hipErrorInvalidValue;
  mcaq_quant_scale q{};
  q.x = input; q.y = output; q.bits = bit_map; q.m = mask; q.xmin = min_vals; q.xmax = max_vals;
  q.B = N; q.C = C; q.H = H; q.W = W; q.ht = n_tiles_h; q.wt = n_tiles_w;
  q.bits_lo = 2; q.nbits = 7;
  q.compat_tile_h = tile_h; q.compat_tile_w = tile_w;
  return mcaq_quant(&q, 1, stream);
}

}  // extern "C"
