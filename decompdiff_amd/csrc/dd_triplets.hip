// Row selection from a CSR built on the device (dd_csr_select_*): the torch_sparse.SparseTensor call site of the reference,
// BondUpdateLayer.triplets (models/encoders/uni_transformer_edge.py:103-123).  The triplet lists (k->j->i) of a directed graph
// are one selection: CSR of the incoming edges of every node (row = target, key = source), select row[e] for every edge e,
// skip the members whose source is col[e].  Op level, not on the sampling path (the fused sampler's bond list is dst-major and
// fully connected: closed-form indices).
//
// Internally int32 (sizes at or above 2^31 are refused by the entry points).  A CSR member is one 64-bit word,
// (key << 32) | entry id: unique, so ordering a run by it is a total order and the result cannot depend on the order in which
// the placement atomics arrived.
#include "dd_common.hpp"

namespace dd {

constexpr int CSR_TB = 256;                       // threads per block of the per-item kernels
constexpr int SCAN_T = 1024, SCAN_I = 4;          // the scan: one block, SCAN_I consecutive items per thread and pass

__device__ __forceinline__ bool csr_in_range(int64_t v, int64_t n) { return (uint64_t)v < (uint64_t)n; }

// deg[row] = entries of the row.  An entry whose row or key is out of range is counted in *bad and belongs to no run (the
// same test keeps it out of k_csr_place): nothing outside the caller's buffers is touched, whatever the ids hold.
__global__ void k_csr_degree(const int64_t* __restrict__ node, const int64_t* __restrict__ key, int E, int64_t n_rows, int64_t n_cols,
                             int32_t* __restrict__ deg, unsigned long long* __restrict__ bad) {
  const long e = (long)blockIdx.x * CSR_TB + threadIdx.x;
  if (e >= E) return;
  const int64_t n = node[e];
  if (csr_in_range(n, n_rows) && csr_in_range(key[e], n_cols)) atomicAdd(&deg[n], 1);
  else atomicAdd(bad, 1ull);
}

// out[i] = in[0] + ... + in[i-1] for i <= n (out may be in: a thread writes the items it read), *total = out[n] in 64 bits.
// One block walks the array SCAN_T * SCAN_I items at a time and carries the running sum: a fixed order, any length, one
// launch.  (A bond graph has 10^3 .. 10^5 edges: a few passes; the decoupled multi-block scan would add launches instead.)
__global__ __launch_bounds__(SCAN_T) void k_scan_exclusive(const int32_t* in, int32_t* out, long n, int64_t* total) {
  __shared__ long long wsum[SCAN_T / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long carry = 0;
  for (long base = 0; base < n; base += SCAN_T * SCAN_I) {
    const long i0 = base + (long)threadIdx.x * SCAN_I;
    int32_t v[SCAN_I];
    long long s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_I; ++k) {
      v[k] = i0 + k < n ? in[i0 + k] : 0;
      s += v[k];
    }
    long long incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SCAN_T / 64; ++w) {
      const long long x = wsum[w];
      if (w < wave) before += x;
      all += x;
    }
    long long ex = carry + before + incl - s;
#pragma unroll
    for (int k = 0; k < SCAN_I; ++k)
      if (i0 + k < n) {
        out[i0 + k] = (int32_t)ex;
        ex += v[k];
      }
    carry += all;
    __syncthreads();                              // wsum is rewritten by the next pass
  }
  if (threadIdx.x == 0) {
    out[n] = (int32_t)carry;
    if (total) *total = carry;
  }
}

// Every entry takes a slot of its row's run (deg counts down to 0): arrival order, put right by k_csr_order.
__global__ void k_csr_place(const int64_t* __restrict__ node, const int64_t* __restrict__ key, int E, int64_t n_rows, int64_t n_cols,
                            const int32_t* __restrict__ ptr, int32_t* __restrict__ deg, uint64_t* __restrict__ tmp) {
  const long e = (long)blockIdx.x * CSR_TB + threadIdx.x;
  if (e >= E) return;
  const int64_t n = node[e], k = key[e];
  if (!csr_in_range(n, n_rows) || !csr_in_range(k, n_cols)) return;
  const int slot = ptr[n] + atomicSub(&deg[n], 1) - 1;
  tmp[slot] = ((uint64_t)(uint32_t)k << 32) | (uint32_t)e;
}

// Order every run by (key, entry id): a member's place is the number of smaller members of its run.  No per-row buffer, so a
// run may have any length; the work is quadratic in it (the lanes of a wave mostly share a run and read the same words), which
// a bond graph's in-degrees of tens to hundreds do not notice.
__global__ void k_csr_order(const int64_t* __restrict__ node, int64_t n_rows, const int32_t* __restrict__ ptr,
                            const uint64_t* __restrict__ tmp, uint64_t* __restrict__ csr) {
  const long p = (long)blockIdx.x * CSR_TB + threadIdx.x;
  if (p >= ptr[n_rows]) return;                    // (entries with ids out of range took no slot)
  const uint64_t mine = tmp[p];
  const int64_t n = node[(uint32_t)mine];
  const int lo = ptr[n], hi = ptr[n + 1];
  int rank = 0;
  for (int q = lo; q < hi; ++q) rank += tmp[q] < mine;
  csr[lo + rank] = mine;
}

__device__ __forceinline__ int csr_lower_bound(const uint64_t* __restrict__ csr, int lo, int hi, uint64_t x) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (csr[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// cnt[r] = members of row sel[r] whose key is not skip[r]; those with that key are one stretch of the ordered run, whose
// start within the run goes to skip_lb[r] (its length is the run's length minus cnt[r]).  A selected row out of range is
// counted in *bad and selects nothing.
__global__ void k_csr_select_count(const int64_t* __restrict__ sel, const int64_t* __restrict__ skip, int R, int64_t n_rows,
                                   int64_t n_cols, const int32_t* __restrict__ ptr, const uint64_t* __restrict__ csr,
                                   int32_t* __restrict__ cnt, int32_t* __restrict__ skip_lb, unsigned long long* __restrict__ bad) {
  const long r = (long)blockIdx.x * CSR_TB + threadIdx.x;
  if (r >= R) return;
  const int64_t n = sel[r];
  int c = 0, lb = 0;
  if (!csr_in_range(n, n_rows)) atomicAdd(bad, 1ull);
  else {
    const int lo = ptr[n], hi = ptr[n + 1];
    c = hi - lo;
    if (skip != nullptr && csr_in_range(skip[r], n_cols)) {
      const uint64_t k0 = (uint64_t)skip[r] << 32;
      const int a = csr_lower_bound(csr, lo, hi, k0), b = csr_lower_bound(csr, a, hi, k0 + (1ull << 32));
      lb = a - lo;
      c -= b - a;
    }
  }
  cnt[r] = c;
  skip_lb[r] = lb;
}

// One thread per surviving member t: its selected row is the last r with off[r] <= t, its place in the run follows from
// t - off[r] and the skipped stretch.  Consecutive lanes write consecutive elements of every list.
__global__ void k_csr_select_fill(const int64_t* __restrict__ sel, const int64_t* __restrict__ skip, int R, int total,
                                  const int32_t* __restrict__ ptr, const uint64_t* __restrict__ csr, const int32_t* __restrict__ off,
                                  const int32_t* __restrict__ skip_lb, int64_t* __restrict__ out_row, int64_t* __restrict__ out_key,
                                  int64_t* __restrict__ out_entry, int64_t* __restrict__ out_sel, int64_t* __restrict__ out_skip) {
  const long t = (long)blockIdx.x * CSR_TB + threadIdx.x;
  if (t >= total || t >= off[R]) return;           // (off[R]: the count call's total -- a larger argument writes nothing more)
  int a = 0, b = R;                                // off[a] <= t < off[b]
  while (b - a > 1) {
    const int mid = a + ((b - a) >> 1);
    if (off[mid] <= t) a = mid;
    else b = mid;
  }
  const int64_t n = sel[a];
  const int lo = ptr[n], m = (int)t - off[a];
  const int skipped = (ptr[n + 1] - lo) - (off[a + 1] - off[a]);
  const uint64_t w = csr[lo + m + (m >= skip_lb[a] ? skipped : 0)];
  if (out_row) out_row[t] = a;
  if (out_key) out_key[t] = (int64_t)(w >> 32);
  if (out_entry) out_entry[t] = (int64_t)(uint32_t)w;
  if (out_sel) out_sel[t] = n;
  if (out_skip) out_skip[t] = skip[a];
}

namespace {
// scratch (bytes): int64 total, int64 bad | int32 deg[n_rows] | int32 ptr[n_rows+1] | u64 tmp[E] | u64 csr[E] |
//                  int32 off[R+1] | int32 skip_lb[R]; every part 8-byte aligned
struct CsrScratch {
  size_t deg, ptr, tmp, csr, off, lb, bytes;
};
inline size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }
bool csr_scratch(int64_t E, int64_t n_rows, int64_t n_cols, int64_t R, CsrScratch* s) {
  const int64_t lim = (int64_t)1 << 31;
  if (E < 0 || n_rows < 0 || n_cols < 0 || R < 0 || E >= lim || n_rows >= lim || n_cols >= lim || R >= lim) return false;
  size_t o = 16;
  s->deg = o; o += pad8(4 * (size_t)n_rows);
  s->ptr = o; o += pad8(4 * ((size_t)n_rows + 1));
  s->tmp = o; o += 8 * (size_t)E;
  s->csr = o; o += 8 * (size_t)E;
  s->off = o; o += pad8(4 * ((size_t)R + 1));
  s->lb = o; o += pad8(4 * (size_t)R);
  s->bytes = o;
  return true;
}
inline dim3 csr_grid(int64_t items) { return dim3((unsigned)((items + CSR_TB - 1) / CSR_TB)); }
}  // namespace

}  // namespace dd

extern "C" size_t dd_csr_select_scratch_bytes(int64_t E, int64_t n_rows, int64_t n_cols, int64_t R) {
  dd::CsrScratch s;
  return dd::csr_scratch(E, n_rows, n_cols, R, &s) ? s.bytes : 0;
}

extern "C" int dd_csr_select_count(const int64_t* node, const int64_t* key, int64_t E, int64_t n_rows, int64_t n_cols,
                                   const int64_t* sel, const int64_t* skip, int64_t R, void* scratch, size_t scratch_bytes,
                                   void* stream) {
  dd::CsrScratch s;
  if (E < 0 || n_rows < 0 || n_cols < 0 || R < 0) return DD_ERR_BAD_ARG;
  if (!dd::csr_scratch(E, n_rows, n_cols, R, &s)) return DD_ERR_UNSUPPORTED_SHAPE;
  if (!scratch || (reinterpret_cast<size_t>(scratch) & 7) != 0 || (E > 0 && (!node || !key)) || (R > 0 && !sel)) return DD_ERR_BAD_ARG;
  if (scratch_bytes < s.bytes) return DD_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  char* base = static_cast<char*>(scratch);
  int64_t* total = reinterpret_cast<int64_t*>(base);
  unsigned long long* bad = reinterpret_cast<unsigned long long*>(base) + 1;
  int32_t* deg = reinterpret_cast<int32_t*>(base + s.deg);
  int32_t* ptr = reinterpret_cast<int32_t*>(base + s.ptr);
  uint64_t* tmp = reinterpret_cast<uint64_t*>(base + s.tmp);
  uint64_t* csr = reinterpret_cast<uint64_t*>(base + s.csr);
  int32_t* off = reinterpret_cast<int32_t*>(base + s.off);
  int32_t* lb = reinterpret_cast<int32_t*>(base + s.lb);
  if (hipMemsetAsync(base, 0, s.ptr, st) != hipSuccess) return DD_ERR_HIP;            // total, bad and deg
  const dim3 block(dd::CSR_TB);
  if (E > 0) hipLaunchKernelGGL(dd::k_csr_degree, dd::csr_grid(E), block, 0, st, node, key, (int)E, n_rows, n_cols, deg, bad);
  hipLaunchKernelGGL(dd::k_scan_exclusive, dim3(1), dim3(dd::SCAN_T), 0, st, deg, ptr, (long)n_rows, (int64_t*)nullptr);
  if (E > 0) {
    hipLaunchKernelGGL(dd::k_csr_place, dd::csr_grid(E), block, 0, st, node, key, (int)E, n_rows, n_cols, ptr, deg, tmp);
    hipLaunchKernelGGL(dd::k_csr_order, dd::csr_grid(E), block, 0, st, node, n_rows, ptr, tmp, csr);
  }
  if (R > 0) hipLaunchKernelGGL(dd::k_csr_select_count, dd::csr_grid(R), block, 0, st, sel, skip, (int)R, n_rows, n_cols, ptr, csr, off, lb, bad);
  hipLaunchKernelGGL(dd::k_scan_exclusive, dim3(1), dim3(dd::SCAN_T), 0, st, off, off, (long)R, total);
  DD_CHECK_LAUNCH();
  return DD_OK;
}

extern "C" int dd_csr_select_fill(const int64_t* sel, const int64_t* skip, int64_t E, int64_t n_rows, int64_t n_cols, int64_t R,
                                  const void* scratch, int64_t total, int64_t* out_row, int64_t* out_key, int64_t* out_entry,
                                  int64_t* out_sel, int64_t* out_skip, void* stream) {
  dd::CsrScratch s;
  if (E < 0 || n_rows < 0 || n_cols < 0 || R < 0 || total < 0) return DD_ERR_BAD_ARG;
  if (!dd::csr_scratch(E, n_rows, n_cols, R, &s) || total >= ((int64_t)1 << 31)) return DD_ERR_UNSUPPORTED_SHAPE;
  if (total == 0) return DD_OK;
  if (!scratch || (reinterpret_cast<size_t>(scratch) & 7) != 0 || !sel || (out_skip && !skip)) return DD_ERR_BAD_ARG;
  const char* base = static_cast<const char*>(scratch);
  hipLaunchKernelGGL(dd::k_csr_select_fill, dd::csr_grid(total), dim3(dd::CSR_TB), 0, (hipStream_t)stream, sel, skip, (int)R, (int)total,
                     reinterpret_cast<const int32_t*>(base + s.ptr), reinterpret_cast<const uint64_t*>(base + s.csr),
                     reinterpret_cast<const int32_t*>(base + s.off), reinterpret_cast<const int32_t*>(base + s.lb), out_row, out_key,
                     out_entry, out_sel, out_skip);
  DD_CHECK_LAUNCH();
  return DD_OK;
}
