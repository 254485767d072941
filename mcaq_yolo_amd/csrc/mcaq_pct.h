// mcaq_pct.h - percentile calibration (core/quantization.py:436-480,
// _calibrate_percentile): the exact q_lo / q_hi quantiles of every channel
// over its B*H*W values, without a sort and without a host sync.
//
// torch.quantile (SURVEY App. A rule 10) takes rank = fp32(q) * (N - 1) and
// interpolates between the order statistics floor(rank) and ceil(rank), so a
// channel needs FOUR order statistics.  They are selected by a three-level
// radix histogram (12 + 10 + 10 bits) over an order-preserving 32-bit key of
// the fp32 value:
//
//   zero     the workspace (histograms, selections, NaN counts)
//   level 0  grid (C, S): histogram of key >> 20 (one per channel)
//   select 0 grid (C): per target, the bin that holds its rank + the rank
//            inside that bin
//   level 1  histogram of (key >> 10) & 0x3ff of the values whose top 12 bits
//            equal a target's bin (one histogram per distinct target prefix)
//   select 1
//   level 2  histogram of key & 0x3ff under the 22-bit prefixes
//   select 2 + the values rebuilt from their keys, the rule-10 lerp, lo / hi
//
// Every level's workgroup holds 4096 counters (level 0: one histogram of
// 4096 bins, levels 1 and 2: four of 1024), 16 KB of LDS, so eight
// workgroups fit a CU.  Workgroups exchange data at kernel boundaries only.
// The counts are integers merged with integer atomicAdd, so every histogram -
// and with it the result - is independent of the order the workgroups arrive
// in.  The workspace is zeroed by a kernel, not a memset: a captured memset
// node did not replay in order with the kernel nodes on the ROCm runtime this
// was developed on (the replayed step returned NaN).
//
// Streaming: a wave owns a chunk of at most 1024 elements of one (image,
// channel) run and has its (up to four) 16-byte loads per lane in flight
// before it touches the histograms.
//
// Contention: a level-0 bin is 1/8 of an octave, so real feature maps pile a
// large share of a channel into a few bins (a SiLU map's plateau at -0.278;
// a constant channel puts all N into one).  hist_add therefore peels the bins
// that neighbouring lanes share into one LDS atomic per wave before the
// remaining lanes add one by one.
#pragma once

namespace mcaq {

constexpr int PCT_TH = 256;
constexpr int PCT_WAVES = PCT_TH / 64;
constexpr int PCT_NT = 4;                       // targets: floor/ceil of the two ranks
constexpr int PCT_B0 = 4096, PCT_B1 = 1024, PCT_B2 = 1024;
constexpr int PCT_CHUNK = 1024;                 // most elements of one run a wave takes at a time
constexpr int PCT_VPL = PCT_CHUNK / 4 / 64;     // 4-element loads per lane and chunk
constexpr int PCT_TARGET_WG = 1024;             // workgroups of a level launch (four per CU)
// workspace words (uint32) of one channel
constexpr int PCT_H0 = 0;
constexpr int PCT_H1 = PCT_H0 + PCT_B0;
constexpr int PCT_H2 = PCT_H1 + PCT_NT * PCT_B1;
constexpr int PCT_SEL = PCT_H2 + PCT_NT * PCT_B2;    // [level][target]{prefix, rank inside}
constexpr int PCT_NAN = PCT_SEL + 3 * PCT_NT * 2;
constexpr int PCT_WORDS = (PCT_NAN + 1 + 3) & ~3;

struct PctArgs {
  const void* x;
  float* lo;
  float* hi;
  unsigned* ws;          // this scale's first channel
  int B, C, HW;
  int cpr, chunk;        // chunks per run, elements per chunk (a multiple of 4, <= PCT_CHUNK)
  unsigned rank[PCT_NT];  // floor(r_lo), ceil(r_lo), floor(r_hi), ceil(r_hi)
  float w[2];             // r_lo - floor(r_lo), r_hi - floor(r_hi)
};

// unsigned key order = value order, -inf .. +inf; -0 folds to +0; every NaN
// takes the largest key (it is still counted, so the ranks stay inside N)
__device__ __forceinline__ unsigned pct_key(float v, bool& nan) {
  unsigned u = __float_as_uint(v);
  nan = v != v;
  if (u == 0x80000000u) u = 0u;
  const unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return nan ? 0xffffffffu : k;
}
__device__ __forceinline__ float pct_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// One count per valid lane into h[bin].  Called by every lane of the wave.
__device__ __forceinline__ void hist_add(unsigned* h, unsigned bin, bool valid, int lane) {
  unsigned long long act = __ballot(valid);
  if (!act) return;
  const int nl = (lane + 1) & 63;
  const unsigned nb = __shfl(bin, nl, 64);
#pragma unroll 1
  for (int r = 0; r < 2; ++r) {
    const bool mine = (act >> lane) & 1ull;
    const unsigned long long cand = __ballot(mine && ((act >> nl) & 1ull) && nb == bin);
    if (!cand) break;
    const int leader = __ffsll((long long)cand) - 1;
    const unsigned lb = __shfl(bin, leader, 64);
    const unsigned long long grp = __ballot(mine && bin == lb);
    if (lane == leader) atomicAdd(&h[lb], (unsigned)__popcll(grp));
    act &= ~grp;
  }
  if ((act >> lane) & 1ull) atomicAdd(&h[bin], 1u);
}

template <int LEVEL> struct PctLevel;
template <> struct PctLevel<0> { static constexpr int NB = PCT_B0, NH = 1, OFF = PCT_H0, SHIFT = 20, PSHIFT = 32; };
template <> struct PctLevel<1> { static constexpr int NB = PCT_B1, NH = PCT_NT, OFF = PCT_H1, SHIFT = 10, PSHIFT = 20; };
template <> struct PctLevel<2> { static constexpr int NB = PCT_B2, NH = PCT_NT, OFF = PCT_H2, SHIFT = 0, PSHIFT = 10; };

// grid (C, S): wave v of workgroup (c, s) takes the chunks 4 s + v,
// 4 (s + S) + v, ... of channel c
template <typename T, int LEVEL>
__global__ __launch_bounds__(PCT_TH) void mcaq_pct_level_kernel(PctArgs a) {
  typedef PctLevel<LEVEL> L;
  __shared__ unsigned h[L::NH * L::NB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int c = blockIdx.x;
  unsigned* ws = a.ws + (size_t)c * PCT_WORDS;
  for (int i = tid; i < L::NH * L::NB; i += PCT_TH) h[i] = 0u;
  // the prefixes of the previous level's selection; a target whose prefix an
  // earlier target has shares that target's histogram (own[t] false)
  unsigned pre[PCT_NT] = {0u, 0u, 0u, 0u};
  bool own[PCT_NT] = {true, false, false, false};
  if (LEVEL > 0) {
#pragma unroll
    for (int t = 0; t < PCT_NT; ++t) {
      pre[t] = ws[PCT_SEL + ((LEVEL - 1) * PCT_NT + t) * 2];
      own[t] = true;
#pragma unroll
      for (int u = 0; u < t; ++u) own[t] = own[t] && pre[u] != pre[t];
    }
  }
  __syncthreads();
  unsigned nnan = 0u;
  auto take = [&](float v, bool valid) {
    bool nan;
    const unsigned k = pct_key(v, nan);
    if constexpr (LEVEL == 0) {
      nnan += (valid && nan) ? 1u : 0u;
      hist_add(h, k >> L::SHIFT, valid, lane);
    } else {
      const unsigned bin = (k >> L::SHIFT) & (unsigned)(L::NB - 1);
      const unsigned p = k >> L::PSHIFT;
      bool m[PCT_NT];
      bool any = false;
#pragma unroll
      for (int t = 0; t < PCT_NT; ++t) { m[t] = valid && own[t] && p == pre[t]; any = any || m[t]; }
      if (!__ballot(any)) return;          // most waves hold no value of a target's bin
#pragma unroll
      for (int t = 0; t < PCT_NT; ++t)
        if (own[t]) hist_add(h + t * L::NB, bin, m[t], lane);
    }
  };
  const int HW = a.HW;
  const int units = a.B * a.cpr;
  for (int u = blockIdx.y * PCT_WAVES + (tid >> 6); u < units; u += gridDim.y * PCT_WAVES) {
    const int b = u / a.cpr, k = u - b * a.cpr;
    const T* run = reinterpret_cast<const T*>(a.x) + ((size_t)b * a.C + c) * HW;
    const int e0 = k * a.chunk, e1 = imin_(HW, e0 + a.chunk);
    const int n = e1 - e0;
    if (n <= 0) continue;                             // wave-uniform
    const T* p = run + e0;
    // scalar head up to the first address a 4-element load may take
    const int mis = (int)(((uintptr_t)p / sizeof(T)) & 3);
    const int head = imin_(n, (4 - mis) & 3);
    const int nvec = (n - head) >> 2;                 // <= 64 * PCT_VPL
    const int tail = n - head - 4 * nvec;
    const T* pv = p + head;
    mcaq_f4v v[PCT_VPL];
#pragma unroll
    for (int j = 0; j < PCT_VPL; ++j) {
      const int q = lane + 64 * j;
      v[j] = mcaq_f4v{0.0f, 0.0f, 0.0f, 0.0f};
      if (q < nvec) v[j] = ElemIO<T>::template ld4<true>(pv + 4 * q);
    }
    float hv = 0.0f, tv = 0.0f;
    if (lane < head) hv = ElemIO<T>::ld(p + lane);
    if (lane < tail) tv = ElemIO<T>::ld(pv + 4 * nvec + lane);
#pragma unroll
    for (int j = 0; j < PCT_VPL; ++j) {
      if (64 * j < nvec) {                            // wave-uniform
        const bool valid = lane + 64 * j < nvec;
        take(v[j].x, valid); take(v[j].y, valid); take(v[j].z, valid); take(v[j].w, valid);
      }
    }
    if (head) take(hv, lane < head);
    if (tail) take(tv, lane < tail);
  }
  __syncthreads();
  unsigned* g = ws + L::OFF;
#pragma unroll
  for (int t = 0; t < L::NH; ++t) {
    if (!own[t]) continue;
    for (int i = tid; i < L::NB; i += PCT_TH) {
      const unsigned cnt = h[t * L::NB + i];
      if (cnt) atomicAdd(&g[t * L::NB + i], cnt);
    }
  }
  if (LEVEL == 0) {
    // one NaN count per wave
    for (int o = 32; o > 0; o >>= 1) nnan += __shfl_xor(nnan, o, 64);
    if (lane == 0 && nnan) atomicAdd(&ws[PCT_NAN], nnan);
  }
}

// grid (C): per target the bin of the level's histogram that holds its rank,
// the prefix extended by that bin and the rank inside the bin - the four
// targets' prefix sums in one scan.  LEVEL 2 also rebuilds the four values
// and writes lo / hi.
template <int LEVEL>
__global__ __launch_bounds__(PCT_TH) void mcaq_pct_select_kernel(PctArgs a) {
  typedef PctLevel<LEVEL> L;
  constexpr int PER = L::NB / PCT_TH;       // consecutive bins of a thread
  __shared__ unsigned part[PCT_NT][PCT_TH];
  __shared__ unsigned keys[PCT_NT];
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  unsigned* ws = a.ws + (size_t)c * PCT_WORDS;
  if (tid < PCT_NT) keys[tid] = 0u;
  unsigned pre[PCT_NT], rank[PCT_NT], sum[PCT_NT];
  const unsigned* g[PCT_NT];
#pragma unroll
  for (int t = 0; t < PCT_NT; ++t) {
    pre[t] = 0u;
    rank[t] = a.rank[t];
    int src = 0;
    if (LEVEL > 0) {
      const unsigned* sel = ws + PCT_SEL + (LEVEL - 1) * PCT_NT * 2;
      pre[t] = sel[t * 2];
      rank[t] = sel[t * 2 + 1];
      src = t;
      for (int u = t - 1; u >= 0; --u) if (sel[u * 2] == pre[t]) src = u;   // the histogram that prefix owns
    }
    g[t] = ws + L::OFF + src * L::NB + tid * PER;
    sum[t] = 0u;
    if (LEVEL > 0 || t == 0) {
#pragma unroll
      for (int i = 0; i < PER; ++i) sum[t] += g[t][i];
    } else {
      sum[t] = sum[0];                       // level 0: one histogram for all four
    }
    part[t][tid] = sum[t];
  }
  __syncthreads();
  for (int d = 1; d < PCT_TH; d <<= 1) {      // inclusive scans
    unsigned v[PCT_NT];
#pragma unroll
    for (int t = 0; t < PCT_NT; ++t) v[t] = tid >= d ? part[t][tid - d] : 0u;
    __syncthreads();
#pragma unroll
    for (int t = 0; t < PCT_NT; ++t) part[t][tid] += v[t];
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < PCT_NT; ++t) {
    unsigned below = part[t][tid] - sum[t];
    if (rank[t] >= below && rank[t] < below + sum[t]) {      // exactly one thread (the counts sum to more than the rank)
      int i = 0;
      for (; i < PER - 1; ++i) {
        const unsigned cnt = g[t][i];
        if (rank[t] < below + cnt) break;
        below += cnt;
      }
      const unsigned full = (LEVEL > 0 ? (pre[t] << 10) : 0u) | (unsigned)(tid * PER + i);
      ws[PCT_SEL + (LEVEL * PCT_NT + t) * 2] = full;
      ws[PCT_SEL + (LEVEL * PCT_NT + t) * 2 + 1] = rank[t] - below;
      if (LEVEL == 2) keys[t] = full;
    }
  }
  if (LEVEL == 2) {
    __syncthreads();
    if (tid < 2) {
      // torch.quantile's lerp (SURVEY App. A rule 10), literally - inf - inf
      // is NaN there too
      const float va = pct_value(keys[2 * tid]), vb = pct_value(keys[2 * tid + 1]);
      const float w = a.w[tid], d = vb - va;
      float r = w < 0.5f ? __builtin_fmaf(w, d, va) : __builtin_fmaf(-d, 1.0f - w, vb);
      if (ws[PCT_NAN]) r = __builtin_nanf("");
      (tid ? a.hi : a.lo)[c] = r;
    }
  }
}

// the workspace zeroed by a launch of its own (a kernel node like the others
// when the sequence is captured); n4: 16-byte words
__global__ __launch_bounds__(PCT_TH) void mcaq_pct_zero_kernel(uint4* __restrict__ ws, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * PCT_TH + threadIdx.x; i < n4; i += (size_t)gridDim.x * PCT_TH)
    ws[i] = make_uint4(0u, 0u, 0u, 0u);
}

template <typename T>
static void pct_launch(const PctArgs& a, int S, hipStream_t stream) {
  const dim3 g(a.C, S), gs(a.C);
  hipLaunchKernelGGL((mcaq_pct_level_kernel<T, 0>), g, dim3(PCT_TH), 0, stream, a);
  hipLaunchKernelGGL(mcaq_pct_select_kernel<0>, gs, dim3(PCT_TH), 0, stream, a);
  hipLaunchKernelGGL((mcaq_pct_level_kernel<T, 1>), g, dim3(PCT_TH), 0, stream, a);
  hipLaunchKernelGGL(mcaq_pct_select_kernel<1>, gs, dim3(PCT_TH), 0, stream, a);
  hipLaunchKernelGGL((mcaq_pct_level_kernel<T, 2>), g, dim3(PCT_TH), 0, stream, a);
  hipLaunchKernelGGL(mcaq_pct_select_kernel<2>, gs, dim3(PCT_TH), 0, stream, a);
}

// ---- the bit map's gradient in the reference's summation order -------------
// The reference's training quantizer (quantization.py:699-727) is an autograd
// graph: x_q += sel ((1 - f) Q_b(x) + f Q_b+1(x)) width by width.  Its
// gradient to the upsampled fraction f(p) is, per pixel,
//     sum_c(g' Q_b+1(x)) - sum_c(g' Q_b(x)),      g' = g m(p) (or g)
// - the two channel sums formed separately by ATen's CPU outer reduction
// (SURVEY App. A rule 1: plain cascade for the columns p < floor(HW/32) 32,
// four interleaved cascades for the tail columns; the other widths add exact
// zeros) - and the nearest-upsampling backward then adds a tile's pixels row
// by row from 0.  These two launches restate exactly that, so grad_bits
// equals the reference's bit for bit; mcaq_qat_backward's own grad_bits is
// the same quantity summed in the kernel's order.
template <typename T>
__global__ __launch_bounds__(PCT_TH) void mcaq_qat_bits_pixel_kernel(mcaq_qat_scale S) {
  const int HW = S.H * S.W;
  const long long i = (long long)blockIdx.x * PCT_TH + threadIdx.x;
  if (i >= (long long)S.B * HW) return;
  const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
  const int h = p / S.W, w = p - h * S.W;
  const float bv = S.bits[((size_t)b * S.ht + nearest_src(h, S.ht, S.H)) * S.wt + nearest_src(w, S.wt, S.W)];
  const int lo = imin_(imax_((int)floorf(bv), QAT_LO), QAT_LO + QAT_NB - 1);
  const int hi = lo < 8 ? lo + 1 : lo;               // Q_hi := Q_lo past 8 bits
  const bool tail = p >= (HW / 32) * 32;
  const bool has_m = S.m != nullptr;
  const float mv = has_m ? S.m[(size_t)b * HW + p] : 1.0f;
  const T* xb = reinterpret_cast<const T*>(S.x) + (size_t)b * S.C * HW + p;
  const float* gb = S.g + (size_t)b * S.C * HW + p;
  auto term = [&](int c, int width) {
    const float g = gb[(size_t)c * HW];
    const float gm = has_m ? g * mv : g;
    return gm * quant_dequant_any(ElemIO<T>::ld(xb + (size_t)c * HW), qparam(S.xmin[c], S.xmax[c], width));
  };
  const float s_hi = aten_sum(S.C, tail, [&](int c) { return term(c, hi); });
  const float s_lo = aten_sum(S.C, tail, [&](int c) { return term(c, lo); });
  S.work[i] = s_hi + (-s_lo);
}

// one thread per tile: its pixels row by row, from 0
__global__ __launch_bounds__(PCT_TH) void mcaq_qat_bits_tile_kernel(mcaq_qat_scale S) {
  const int i = blockIdx.x * PCT_TH + threadIdx.x;
  if (i >= S.B * S.ht * S.wt) return;
  const int tw = i % S.wt, th = (i / S.wt) % S.ht, b = i / (S.wt * S.ht);
  const int h0 = band_start(th, S.ht, S.H), h1 = band_start(th + 1, S.ht, S.H);
  const int w0 = band_start(tw, S.wt, S.W), w1 = band_start(tw + 1, S.wt, S.W);
  const float* pix = S.work + (size_t)b * S.H * S.W;
  float acc = 0.0f;
  for (int h = h0; h < h1; ++h)
    for (int w = w0; w < w1; ++w) acc = acc + pix[(size_t)h * S.W + w];
  S.gb[i] = acc;
}

}  // namespace mcaq

extern "C" {

int mcaq_qat_bits_gradient(const mcaq_qat_scale* scales, int nscales, hipStream_t stream) {
  using namespace mcaq;
  if (!scales || nscales < 1 || nscales > 3) return (int)hipErrorInvalidValue;
  for (int i = 0; i < nscales; ++i) {
    const mcaq_qat_scale& s = scales[i];
    if (!s.x || !s.g || !s.bits || !s.xmin || !s.xmax || !s.gb || !s.work) return (int)hipErrorInvalidValue;
    if (s.B < 1 || s.C < 1 || s.H < 1 || s.W < 1 || s.ht < 1 || s.wt < 1 || s.ht > s.H || s.wt > s.W)
      return (int)hipErrorInvalidValue;
    if ((long long)s.B * s.H * s.W >= (1ll << 31) || s.dtype < MCAQ_DTYPE_F32 || s.dtype > MCAQ_DTYPE_BF16)
      return (int)hipErrorInvalidValue;
  }
  for (int i = 0; i < nscales; ++i) {
    const mcaq_qat_scale& s = scales[i];
    const long long np = (long long)s.B * s.H * s.W;
    const dim3 g((unsigned)((np + PCT_TH - 1) / PCT_TH));
    switch (s.dtype) {
      case MCAQ_DTYPE_F32: hipLaunchKernelGGL(mcaq_qat_bits_pixel_kernel<float>, g, dim3(PCT_TH), 0, stream, s); break;
      case MCAQ_DTYPE_F16: hipLaunchKernelGGL(mcaq_qat_bits_pixel_kernel<_Float16>, g, dim3(PCT_TH), 0, stream, s); break;
      default: hipLaunchKernelGGL(mcaq_qat_bits_pixel_kernel<Bf16>, g, dim3(PCT_TH), 0, stream, s); break;
    }
    const int nt = s.B * s.ht * s.wt;
    hipLaunchKernelGGL(mcaq_qat_bits_tile_kernel, dim3((nt + PCT_TH - 1) / PCT_TH), dim3(PCT_TH), 0, stream, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

size_t mcaq_percentile_workspace_bytes(int C) {
  return C < 1 ? 0 : (size_t)C * mcaq::PCT_WORDS * sizeof(unsigned);
}

int mcaq_percentile(const mcaq_percentile_scale* scales, int nscales, void* workspace, size_t workspace_bytes,
                    hipStream_t stream) {
  using namespace mcaq;
  if (!scales || nscales < 1 || nscales > MCAQ_MAX_SEGMENTS || !workspace) return (int)hipErrorInvalidValue;
  long long ctot = 0;
  for (int i = 0; i < nscales; ++i) {
    const mcaq_percentile_scale& s = scales[i];
    if (!s.x || !s.lo || !s.hi || s.B < 1 || s.C < 1 || s.H < 1 || s.W < 1) return (int)hipErrorInvalidValue;
    const long long HW = (long long)s.H * s.W, N = HW * s.B;
    // fp32(q) * (N - 1) is exact rank arithmetic only below 2^24 values
    if (HW >= (1ll << 24) || N >= (1ll << 24)) return (int)hipErrorInvalidValue;
    if (!(s.q_lo >= 0.0f && s.q_lo <= 1.0f && s.q_hi >= 0.0f && s.q_hi <= 1.0f)) return (int)hipErrorInvalidValue;
    if (s.dtype < MCAQ_DTYPE_F32 || s.dtype > MCAQ_DTYPE_BF16) return (int)hipErrorInvalidValue;
    ctot += s.C;
  }
  if (ctot > (1 << 20) || workspace_bytes < mcaq_percentile_workspace_bytes((int)ctot)) return (int)hipErrorInvalidValue;
  if ((uintptr_t)workspace & 15) return (int)hipErrorInvalidValue;
  const size_t n4 = mcaq_percentile_workspace_bytes((int)ctot) / sizeof(uint4);
  const size_t zb = (n4 + PCT_TH - 1) / PCT_TH;
  hipLaunchKernelGGL(mcaq_pct_zero_kernel, dim3((unsigned)(zb < 2048 ? zb : 2048)), dim3(PCT_TH), 0, stream,
                     static_cast<uint4*>(workspace), n4);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  unsigned* ws = static_cast<unsigned*>(workspace);
  for (int i = 0; i < nscales; ++i) {
    const mcaq_percentile_scale& s = scales[i];
    PctArgs a;
    a.x = s.x; a.lo = s.lo; a.hi = s.hi; a.ws = ws;
    a.B = s.B; a.C = s.C; a.HW = s.H * s.W;
    const int N = s.B * a.HW;
    const float qs[2] = {s.q_lo, s.q_hi};
    for (int j = 0; j < 2; ++j) {
      volatile float rank = qs[j] * (float)(N - 1);      // one fp32 product, as torch.quantile's
      const float fl = floorf(rank), ce = ceilf(rank);
      unsigned lo = (unsigned)fl, hi = (unsigned)ce;
      if (hi > (unsigned)(N - 1)) hi = (unsigned)(N - 1);   // q = 1: the product may round up
      if (lo > hi) lo = hi;
      a.rank[2 * j] = lo;
      a.rank[2 * j + 1] = hi;
      a.w[j] = rank - fl;
    }
    // a run in chunks of equal size (a multiple of 4 elements, so the chunks
    // of an aligned run stay aligned), one wave a chunk
    a.cpr = (a.HW + PCT_CHUNK - 1) / PCT_CHUNK;
    a.chunk = (((a.HW + a.cpr - 1) / a.cpr) + 3) & ~3;
    const long long units = (long long)s.B * a.cpr;
    // whole rounds of chunks per wave, about PCT_TARGET_WG workgroups a launch
    const long long per_round = (long long)PCT_WAVES * PCT_TARGET_WG;
    const long long rounds = (units * s.C + per_round - 1) / per_round;
    long long S = (units + PCT_WAVES * rounds - 1) / (PCT_WAVES * rounds);
    if (S < 1) S = 1;
    if (S > 65535) S = 65535;
    switch (s.dtype) {
      case MCAQ_DTYPE_F32: pct_launch<float>(a, (int)S, stream); break;
      case MCAQ_DTYPE_F16: pct_launch<_Float16>(a, (int)S, stream); break;
      default: pct_launch<Bf16>(a, (int)S, stream); break;
    }
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    ws += (size_t)s.C * PCT_WORDS;
  }
  return 0;
}

}  // extern "C"
