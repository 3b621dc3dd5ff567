// Graph construction and light per-node / per-edge kernels:
//   k_knn            torch_cluster.knn via torch_geometric.nn.knn_graph (uni_transformer_edge.py:353)
//   k_knn_csr        the same call on a flat batch of different samples (op level: functional.knn_graph)
//   k_edge_weights   e_w = sigmoid(MLP_{20->128->1}(G(dist)))           (uni_transformer_edge.py:422-427)
//   k_embed_*        atom / bond embeddings + context composition        (decompdiff.py:219-256,279,296-297)
//   k_bl_assemble3   per-bond-edge partial sums of the bond_layer first Linear (packing.py docstring)
// One wavefront (64 lanes) per centre / edge row; feature rows are 128 floats = 2 per lane,
// so every gather is a single coalesced 512-byte row read.
#include <type_traits>

#include "dd_kernels.hpp"

namespace dd {

// ------------------------------------------------------------------------------------ kNN
// One wave per centre, K <= 64 neighbours.  Each lane owns candidates c = lane, lane+64, ... (<= 32 per lane,
// N <= 2048).  Key = (bits(d2) << 32) | index is monotone in (d2, index) because d2 >= 0: the K
// smallest keys in ascending order are the neighbours in ascending (distance, index) — the same
// total order the oracle's stable sort uses.  d2 = (dx*dx + dy*dy) + dz*dz with no FMA contraction.
// The per-lane candidate count is a template parameter (ceil(N / 64), not the maximum 16).

// atom n of sample b is real (not padding): protein rows n < NP count up to np_real[b], ligand rows up to nl_real[b]
__device__ __forceinline__ bool atom_is_real(int n, int NP, int npb, int nlb) { return n < NP ? n < npb : (n - NP) < nlb; }

// Positions of one sample, either one [N,3] block (the workspace copy: l = p + 3 NP) or the sampler's separate protein /
// ligand blocks (the fused head launch reads x_t where the step kernel left it: same values, other addresses).
struct PosView {
  const float* p;
  const float* l;
  int NP;
  __device__ __forceinline__ float get(int n, int c) const { return n < NP ? p[3 * n + c] : l[3 * (n - NP) + c]; }
};
__device__ __forceinline__ PosView pos_view(const GraphArgs& a, int b) {   // sample b of the problem (GraphArgs: both forms)
  return PosView{a.prot + (long)b * a.prot_stride, a.lig + (long)b * a.lig_stride, a.NP};
}
// ... of a problem known to be one [B, N, 3] block at a.prot (k_knn, k_edge_weights2): with l = p + 3 NP in sight the compiler
// folds PosView::get into one address
__device__ __forceinline__ PosView block_view(const GraphArgs& a, int b) {
  const float* xb = a.prot + (long)b * (a.NP + a.NL) * 3;
  return PosView{xb, xb + 3 * (long)a.NP, a.NP};
}

// One wave: the K nearest neighbours of centre i, ascending (d2, index), to nbr_row[0..K) (global) and -- when srt is
// given -- to srt[0..K) (this wave's LDS slice: the edge-weight pass of the fused head launch reads them from there).
template <int CAND>
__device__ __forceinline__ void knn_wave(const PosView& pv, int i, int N, int K, int32_t* __restrict__ nbr_row, bool masked, int npb,
                                         int nlb, unsigned long long* sel /*LDS, 64 per wave*/, int32_t* srt /*LDS or nullptr*/) {
  const int lane = threadIdx.x & 63;
  const float cx = pv.get(i, 0), cy = pv.get(i, 1), cz = pv.get(i, 2);
  unsigned khi[CAND], klo[CAND];                         // key = (bits(d2), index): d2 >= 0, so unsigned order = float order
#pragma unroll
  for (int t = 0; t < CAND; ++t) {
    const int c = lane + 64 * t;
    khi[t] = ~0u; klo[t] = ~0u;
    if (c < N && c != i && (!masked || atom_is_real(c, pv.NP, npb, nlb))) {
      float dx = __fsub_rn(cx, pv.get(c, 0)), dy = __fsub_rn(cy, pv.get(c, 1)), dz = __fsub_rn(cz, pv.get(c, 2));
      float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
      khi[t] = __float_as_uint(d2); klo[t] = (unsigned)c;
    }
  }
  // Selection without K serial wave-min rounds:
  //  (1) radix select on the distance bits: the K-th smallest d2 (with multiplicity), one bit per trip from the top;
  //      a trip is CAND ballots + scalar popcounts, no cross-lane dependency chain;
  //  (2) every candidate below that distance is a neighbour, and of those AT it the `need` lowest indices (candidate
  //      c = lane + 64 t, so index order is (t, lane) order: ballot prefix counts);
  //  (3) the K selected keys go to LDS, one per slot, and lane j ranks key j among them: its position in ascending
  //      (d2, index) order -- the order K rounds of wave-min produced (and the oracle's stable sort).
  unsigned prefix = 0;
  int need = K;
  for (int bit = 31; bit >= 0; --bit) {
    int c0 = 0;                                          // keys that agree with the prefix above `bit` and have this bit clear
#pragma unroll
    for (int t = 0; t < CAND; ++t)
      c0 += __builtin_popcountll(__builtin_amdgcn_ballot_w64((khi[t] >> bit) == (prefix >> bit)));
    if (c0 < need) { need -= c0; prefix |= 1u << bit; }
  }
  int base = 0, ties = 0;
#pragma unroll
  for (int t = 0; t < CAND; ++t) {
    const bool eq = khi[t] == prefix;
    const unsigned long long meq = __builtin_amdgcn_ballot_w64(eq);
    const int tie_rank = ties + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(meq >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)meq, 0u));
    const bool take = khi[t] < prefix || (eq && tie_rank < need);
    const unsigned long long mtk = __builtin_amdgcn_ballot_w64(take);
    const int slot = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mtk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mtk, 0u));
    if (take && slot < 64) sel[slot] = ((unsigned long long)khi[t] << 32) | klo[t];
    base += __builtin_popcountll(mtk);
    ties += __builtin_popcountll(meq);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // this wave's LDS writes before its reads below (one wave owns the slice)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (lane < K) {
    const unsigned long long mine = sel[lane];
    int rank = 0;
    for (int j = 0; j < K; ++j) rank += sel[j] < mine ? 1 : 0;     // same address for every lane: an LDS broadcast
    const int32_t idx = (int32_t)(unsigned)(mine & 0xffffffffull);
    nbr_row[rank] = idx;
    if (srt) srt[rank] = idx;
  }
  if (srt) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
}

template <int CAND>
__global__ __launch_bounds__(256) void k_knn(const GraphArgs a) {
  __shared__ unsigned long long sel[4][64];
  const int N = a.NP + a.NL, lane = threadIdx.x & 63;
  const int centre = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (centre >= a.B * N) return;
  const int b = centre / N, i = centre % N;
  const bool masked = a.nl_real != nullptr;
  const int npb = masked && a.np_real ? a.np_real[b] : a.NP, nlb = masked ? a.nl_real[b] : a.NL;
  if (masked && !atom_is_real(i, a.NP, npb, nlb)) {        // a padding atom is no centre: its list is never read
    if (lane < a.K) a.nbr[(long)centre * a.K + lane] = 0;
    return;
  }
  knn_wave<CAND>(block_view(a, b), i, N, a.K, a.nbr + (long)centre * a.K, masked, npb, nlb, sel[threadIdx.x >> 6], nullptr);
}

// ------------------------------------------------------------------- kNN over a flat, ragged batch
// torch_geometric.nn.knn_graph on a PyG Batch of DIFFERENT complexes: x is one flat [n,3] tensor, sample b owns rows
// ptr[b] .. ptr[b+1]-1 (any count, 0 and 1 included) and its centres get k_b = min(K, n_b - 1) neighbours (loop: the centre is a
// candidate too, k_b = min(K, n_b)).  One wave per centre row, the same key and the same total order as knn_wave -- a dense batch
// gives the lists of k_knn -- but the candidates are STREAMED: chunks of 64 * CAND rows (<= 2048), and the k_b best keys so far
// ride along in registers as one more candidate per lane (lane j: the j-th smallest, so ties among them are in index order,
// and they come before the chunk's candidates in the tie order because their indices are lower).  Every chunk is then the
// selection of knn_wave over CAND + 1 candidates per lane; the result is exact for every n_b.  The first chunk holds at least
// k_b real candidates (64 * CAND - 1 >= 64 when the sample is longer than a chunk), so from then on k_b real keys are carried.
// The wave writes its k_b edges as global int64 rows into the compact [2,E] edge_index (row 0 neighbour, row 1 centre) at
// out_off[b] + i * k_b.  ptr / out_off are read defensively: rows or edges outside [0,n) / [0,E) are never touched.
template <int CAND>
__global__ __launch_bounds__(256) void k_knn_csr(const float* __restrict__ x, const int32_t* __restrict__ ptr, int B, int n, int K,
                                                 int loop, const int64_t* __restrict__ out_off, long E,
                                                 int64_t* __restrict__ edge_index) {
  __shared__ unsigned long long sel_all[4][64], srt_all[4][64];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform: the sample search is scalar)
  unsigned long long* sel = sel_all[w];
  unsigned long long* srt = srt_all[w];
  const int r = blockIdx.x * 4 + w;                        // centre: global row
  if (r >= n) return;
  int lo = 0, hi = B - 1;                                  // the sample with ptr[b] <= r < ptr[b+1] (empty samples are skipped)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid + 1] <= r) lo = mid + 1; else hi = mid;
  }
  const int s0 = ptr[lo], s1 = min(ptr[lo + 1], n);
  const int nb = s1 - s0, i = r - s0;
  if (s0 < 0 || i < 0 || i >= nb) return;
  const int kb = min(K, loop ? nb : nb - 1);
  if (kb <= 0) return;
  const long pos = (long)out_off[lo] + (long)i * kb;
  if (pos < 0 || pos + kb > E) return;
  const float* xs = x + 3 * (long)s0;
  const float cx = xs[3 * i], cy = xs[3 * i + 1], cz = xs[3 * i + 2];
  unsigned chi = ~0u, clo = ~0u;                           // carried key of this lane (none yet)
  for (int c0 = 0; c0 < nb; c0 += 64 * CAND) {
    unsigned khi[CAND], klo[CAND];
#pragma unroll
    for (int t = 0; t < CAND; ++t) {
      const int c = c0 + lane + 64 * t;
      khi[t] = ~0u; klo[t] = ~0u;
      if (c < nb && (loop || c != i)) {
        float dx = __fsub_rn(cx, xs[3 * (long)c]), dy = __fsub_rn(cy, xs[3 * (long)c + 1]), dz = __fsub_rn(cz, xs[3 * (long)c + 2]);
        float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
        khi[t] = __float_as_uint(d2); klo[t] = (unsigned)c;
      }
    }
    // (1) radix select of the k_b-th smallest distance among carried + chunk keys
    unsigned prefix = 0;
    int need = kb;
    for (int bit = 31; bit >= 0; --bit) {
      int n0 = __builtin_popcountll(__builtin_amdgcn_ballot_w64((chi >> bit) == (prefix >> bit)));
#pragma unroll
      for (int t = 0; t < CAND; ++t)
        n0 += __builtin_popcountll(__builtin_amdgcn_ballot_w64((khi[t] >> bit) == (prefix >> bit)));
      if (n0 < need) { need -= n0; prefix |= 1u << bit; }
    }
    // (2) keys below it, and of those at it the `need` lowest indices: carried keys first, then (t, lane) order
    int base = 0, ties = 0;
    auto place = [&](unsigned h, unsigned l) {
      const bool eq = h == prefix;
      const unsigned long long meq = __builtin_amdgcn_ballot_w64(eq);
      const int tie_rank = ties + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(meq >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)meq, 0u));
      const bool take = h < prefix || (eq && tie_rank < need);
      const unsigned long long mtk = __builtin_amdgcn_ballot_w64(take);
      const int slot = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mtk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mtk, 0u));
      if (take && slot < 64) sel[slot] = ((unsigned long long)h << 32) | l;
      base += __builtin_popcountll(mtk);
      ties += __builtin_popcountll(meq);
    };
    place(chi, clo);
#pragma unroll
    for (int t = 0; t < CAND; ++t) place(khi[t], klo[t]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // this wave's LDS writes before its reads below (one wave owns the slices)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // (3) rank the k_b selected keys: lane j carries the j-th smallest into the next chunk
    if (lane < kb) {
      const unsigned long long mine = sel[lane];
      int rank = 0;
      for (int j = 0; j < kb; ++j) rank += sel[j] < mine ? 1 : 0;
      srt[rank] = mine;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const unsigned long long s = lane < kb ? srt[lane] : ~0ull;
    chi = (unsigned)(s >> 32); clo = (unsigned)(s & 0xffffffffull);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // ... and these reads before the next chunk's writes
    __builtin_amdgcn_wave_barrier();
  }
  if (lane < kb) {
    edge_index[pos + lane] = (int64_t)s0 + (int64_t)clo;
    edge_index[E + pos + lane] = (int64_t)r;
  }
}

// ------------------------------------------------------------------------------ edge weights
// One wave per node, 16 neighbours per tile in the attention kernels' k-pass layout
// (lane = (member mm, channel group cg), 32 hidden channels per lane).  hidden = b1 + W1 . G(d) is 5 k-steps of
// v_mfma_f32_16x16x4_f32 with the weights as A operands held in 40 registers; LayerNorm + ReLU and the 128 -> 1
// output layer reduce over the 4 lanes of a member with permlane swaps.
typedef float f32x4e __attribute__((ext_vector_type(4)));
// The 128-channel vectors of the edge-weight MLP (first-layer bias, LayerNorm gamma / beta, output weights) in LDS, once per
// workgroup: kept in registers they cost 128 VGPRs per lane for two uses each, which left the kernel at ONE wave per SIMD.
__device__ __forceinline__ void ew_stage(float* lw /*LDS, 512 floats*/, const float* __restrict__ b1, const float* __restrict__ ln,
                                         const float* __restrict__ w2) {
  const int t = threadIdx.x;                             // 256 threads: 128 float4
  if (t < 32) reinterpret_cast<float4*>(lw)[t] = reinterpret_cast<const float4*>(b1)[t];
  else if (t < 96) reinterpret_cast<float4*>(lw + 128)[t - 32] = reinterpret_cast<const float4*>(ln)[t - 32];   // gamma | beta
  else if (t < 128) reinterpret_cast<float4*>(lw + 384)[t - 96] = reinterpret_cast<const float4*>(w2)[t - 96];
}
// One wave: e_w of the K edges of node i.  nbr_row: the node's neighbour list (global memory, or the LDS copy knn_wave left).
__device__ __forceinline__ void ew_wave(const PosView& pv, int i, int K, const int32_t* nbr_row, const float* __restrict__ W1T,
                                        const float* lw /*LDS: ew_stage*/, const float* __restrict__ b2, float* __restrict__ ew_row) {
  const int lane = threadIdx.x & 63, mm = lane & 15, cg = lane >> 4;
  const float cx = pv.get(i, 0), cy = pv.get(i, 1), cz = pv.get(i, 2);
  float Wa[5][8];                                        // A operands: W1T[4s + cg][16nt + mm]
#pragma unroll
  for (int s = 0; s < 5; ++s)
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) Wa[s][nt] = W1T[(4 * s + cg) * 128 + 16 * nt + mm];
  const float bias2 = b2[0];
  auto quad = [](float v) { v = swap16_sum(v, v); return swap32_sum(v, v); };
  for (int t0 = 0; t0 < K; t0 += 16) {
    // (the LDS offset is made opaque per trip: the vectors are loop-invariant, and hoisted out of the loop they are the
    // 128 registers per lane this layout is there to avoid)
    int o4 = 4 * cg;
    asm volatile("" : "+v"(o4));
    auto vec = [&](int which, int nt) { return *reinterpret_cast<const float4*>(lw + which * 128 + 16 * nt + o4); };   // channels 16nt + 4cg .. +3
    const int m = t0 + mm;
    const int j = nbr_row[m < K ? m : K - 1];
    const float dx = cx - pv.get(j, 0), dy = cy - pv.get(j, 1), dz = cz - pv.get(j, 2);
    const float d = sqrtf(dx * dx + dy * dy + dz * dz);
    f32x4e acc[8];
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) { const float4 bb = vec(0, nt); acc[nt] = f32x4e{bb.x, bb.y, bb.z, bb.w}; }
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const float fk = gauss_feat(d, 4 * s + cg);
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Wa[s][nt], fk, acc[nt], 0, 0, 0);
    }
    float sum = 0.f;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) sum += (acc[nt][0] + acc[nt][1]) + (acc[nt][2] + acc[nt][3]);
    const float mean = quad(sum) * (1.0f / 128.0f);
    float var = 0.f;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) { acc[nt][r] -= mean; var = fmaf(acc[nt][r], acc[nt][r], var); }
    const float rstd = dd_rsqrt(quad(var) * (1.0f / 128.0f) + 1e-5f);
    float dot = 0.f;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
      const float4 gm = vec(1, nt), bt = vec(2, nt), ww = vec(3, nt);
      dot = fmaf(fmaxf(fmaf(acc[nt][0] * rstd, gm.x, bt.x), 0.f), ww.x, dot);
      dot = fmaf(fmaxf(fmaf(acc[nt][1] * rstd, gm.y, bt.y), 0.f), ww.y, dot);
      dot = fmaf(fmaxf(fmaf(acc[nt][2] * rstd, gm.z, bt.z), 0.f), ww.z, dot);
      dot = fmaf(fmaxf(fmaf(acc[nt][3] * rstd, gm.w, bt.w), 0.f), ww.w, dot);
    }
    const float logit = quad(dot) + bias2;
    if (cg == 0 && m < K) ew_row[m] = 1.0f / (1.0f + expf(-logit));
  }
}
__global__ __launch_bounds__(256, 3) void k_edge_weights2(const GraphArgs a) {
  __shared__ __attribute__((aligned(16))) float lw[512];
  ew_stage(lw, a.EW_b1, a.EW_ln, a.EW_w2);
  __syncthreads();                                       // (before any wave leaves)
  const int N = a.NP + a.NL;
  const int node = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (node >= a.B * N) return;
  const int b = node / N, i = node % N;
  if (a.nl_real != nullptr && !atom_is_real(i, a.NP, a.np_real ? a.np_real[b] : a.NP, a.nl_real[b])) return;   // padding atom
  ew_wave(block_view(a, b), i, a.K, a.nbr + (long)node * a.K, a.EW_W1T, lw, a.EW_b2, a.ew + (long)node * a.K);
}

// -------------------------------------------------------------------------------- embeddings
// protein_h[r, c] = sum_f W[c, f] * feat[r, f] + b[c]     (W padded to 128 rows: row 127 = 0, b[127] = 0)
__global__ void k_embed_protein(const float* __restrict__ feat, int rows, const float* __restrict__ W,
                                const float* __restrict__ b, float* __restrict__ out) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * 128) return;
  int r = idx >> 7, c = idx & 127;
  float acc = 0.f;
  const float* f = feat + (long)r * 29;
  const float* w = W + c * 29;
#pragma unroll
  for (int k = 0; k < 29; ++k) acc = fmaf(w[k], f[k], acc);
  out[idx] = acc + b[c];
}

// One launch at the head of a step: node embedding / context, bond embedding, and the per-forward work counters
// of the persistent kernels (64 ints) set to zero.
__device__ __forceinline__ void embed_block(const unsigned blk, const EmbedArgs& e) {
  // (measurement build: + the tile-queue schedule's flag words; the error word behind them is sticky: dd_queue_error reads
  // and clears it.  The default library has no such schedule and zeroes the work counters only.)
#if defined(DD_DEBUG_OPTIONS) && DD_DEBUG_OPTIONS
  constexpr int n_zero = DD_NUM_COUNTERS + DD_FLAG_ERR;
#else
  constexpr int n_zero = DD_NUM_COUNTERS;
#endif
  if (blk == 0 && e.counters)
    for (int i = threadIdx.x; i < n_zero; i += 256) e.counters[i] = 0;
  // the step index moves on with the first launch of a step's forward (nothing before the step kernels reads it): the
  // step kernels use *advance - 1, and no one-thread launch sits at the end of a step
  if (blk == 0 && threadIdx.x == 64 && e.advance) *e.advance += 1;
  const int NP = e.NP, NL = e.NL, nv = e.nv;
  if ((int)blk < e.node_blocks) {
    const int N = NP + NL;
    const long idx = (long)blk * 256 + threadIdx.x;
    if (idx >= (long)e.B * N * 128) return;
    const int c = idx & 127;
    const long node = idx >> 7;
    const int b = node / N, n = node % N;
    float val;
    if (n < NP) {
      val = e.protein_h[((long)b * NP + n) * 128 + c];
    } else {
      const long a = (long)b * NL + (n - NP);
      const float* w = e.Wl + c * (nv + 2);              // ligand_atom_emb row: nv class columns + 2 arm / scaffold indicators
      val = w[e.lig_v[a]] + w[nv] * e.lig_aux[2 * a] + w[nv + 1] * e.lig_aux[2 * a + 1] + e.bl[c];
    }
    e.h[idx] = val;
    if (c < 3) {
      const float p = n < NP ? e.protein_pos[((long)b * NP + n) * 3 + c] : e.lig_pos[((long)b * NL + (n - NP)) * 3 + c];
      e.xa[node * 3 + c] = p;
      e.xb[node * 3 + c] = p;
    }
  } else {
    const long idx = (long)(blk - e.node_blocks) * 256 + threadIdx.x;
    if (idx >= e.bond_rows * 128) return;
    const int c = idx & 127;
    const long r = idx >> 7;
    e.hb[idx] = e.Wb[c * 5 + e.bond[r]] + e.bb[c];
  }
}
__global__ __launch_bounds__(256) void k_embed_all(const EmbedArgs e) { embed_block(blockIdx.x, e); }

// --------------------------------------------------------------------------- layer-0 rows from tables
// One thread per float4 of an output row.  Ligand atom a = b*NL + i with combination c = 8*(arm flag) + class:
//   l0_P[b*N + NP + i] = TN[c] (640), PL[a] = TL[c] (1280), l0_qn[b*N + NP + i] = TQN[c], qlnb[a] = TQL[c];
// bond e = b*Eb + t*(NL-1) + s' of type ty with destination atom t:  PB[e] = TB[ty] (640), qb[e] = TQB[c(t)][ty].
constexpr int L0_TN = 0, L0_TL = 16 * 640, L0_TB = L0_TL + 16 * 1280, L0_TQN = L0_TB + 5 * 640, L0_TQL = L0_TQN + 16 * 128,
              L0_TQB = L0_TQL + 16 * 128;
// PLW: floats of a PL row the model fills -- 1280, or 640 for the narrow bond layer (the node_layer_with_bond blocks; the table
// rows and the PL rows keep their 1280-float stride, columns [640, 1280) are not copied)
template <int PLW>
__device__ __forceinline__ void layer0_rows_block(const unsigned blk, const Layer0RowsArgs& r) {
  const long idx = (long)blk * 256 + threadIdx.x;
  const int NP = r.NP, NL = r.NL, N = NP + NL, Eb = NL * (NL - 1);
  auto combo = [&](long a) { return (r.lig_aux[2 * a + 1] > 0.5f ? 8 : 0) + r.lig_v[a]; };
  const float4* t4 = reinterpret_cast<const float4*>(r.tab);
  if (idx < r.atom_f4) {
    constexpr int PER = l0_atom_f4(PLW), K1 = 160 + PLW / 4, K2 = K1 + 32;
    static_assert(PLW != 1280 || (PER == DD_L0_ATOM_F4 && K1 == 480 && K2 == 512), "wide layout");
    const long a = idx / PER;
    const int k = (int)(idx % PER);
    const int b = (int)(a / NL), i = (int)(a % NL);
    const int c = combo(a);
    const long node = (long)b * N + NP + i;
    if (k < 160) reinterpret_cast<float4*>(r.l0_P + node * 640)[k] = t4[(L0_TN + c * 640) / 4 + k];
    else if (k < K1) reinterpret_cast<float4*>(r.PL + a * 1280)[k - 160] = t4[(L0_TL + c * 1280) / 4 + (k - 160)];
    else if (k < K2) reinterpret_cast<float4*>(r.l0_qn + node * 128)[k - K1] = t4[(L0_TQN + c * 128) / 4 + (k - K1)];
    else reinterpret_cast<float4*>(r.qlnb + a * 128)[k - K2] = t4[(L0_TQL + c * 128) / 4 + (k - K2)];
    return;
  }
  constexpr int PERB = DD_L0_BOND_F4;
  const long j = idx - r.atom_f4;
  const long e = j / PERB;
  if (e >= (long)r.B * Eb) return;
  const int k = (int)(j % PERB);
  const int ty = r.bond[e];
  if (k < 160) {
    reinterpret_cast<float4*>(r.PB + e * 640)[k] = t4[(L0_TB + ty * 640) / 4 + k];
  } else {
    const int b = (int)(e / Eb), t = (int)((e % Eb) / (NL - 1));
    const int c = combo((long)b * NL + t);
    reinterpret_cast<float4*>(r.qb + e * 128)[k - 160] = t4[(L0_TQB + (c * 5 + ty) * 128) / 4 + (k - 160)];
  }
}
template <int PLW>
__global__ __launch_bounds__(256) void k_layer0_rows(const Layer0RowsArgs r) { layer0_rows_block<PLW>(blockIdx.x, r); }

// ------------------------------------------------------------------------------ head of a forward: two launches
// Everything the first attention layer waits for that only depends on the state the previous reverse step left:
// k_graph -- the kNN graph + edge weights, one wave per centre (the bodies of k_knn and k_edge_weights2, the list
// handed over through LDS; x_t is read from the sampler's protein / ligand position buffers, so the launch does not
// wait for the workspace copy the embedding blocks write); k_head_rows -- the embeddings / context (with the zeroed work
// counters and the step index) and the layer-0 rows (the bodies of k_embed_all and k_layer0_rows as two block ranges).
// Outputs bit-identical to the four separate launches.
//
// Block boundary: a refine net with num_blocks > 1 rebuilds the kNN graph and the edge weights from the CURRENT context
// coordinates before every block but the first (uni_transformer_edge.py:402-427).  That is the same k_graph launch on one
// [B, N, 3] block of the workspace (w.xa / w.xb, whichever holds x behind the previous block's last layer) instead of the
// sampler's separate buffers: the two differ in the GraphArgs' base pointers and strides only, so equal coordinates give the
// same nbr rows and the same e_w bits as the head's launch.  Padding atoms are neither centres nor candidates.
// All N atoms are candidates again.  The protein-protein distances do not change between blocks, but that is not exploited:
// a centre's list is ONE selection over protein and ligand candidates in (distance, index) order, so a protein centre near
// the ligand needs the moved ligand atoms ranked among its protein neighbours anyway (EXPERIMENTS.md).
// KW: the width of the LDS hand-off srt -- 32 for K <= 32 (the shipped graph), 64 for K <= DD_KNN_MAX
template <int CAND, int KW>
__global__ __launch_bounds__(256, 3) void k_graph(const GraphArgs a) {
  __shared__ unsigned long long sel[4][64];
  __shared__ int32_t srt[4][KW];
  __shared__ __attribute__((aligned(16))) float lw[512];
  ew_stage(lw, a.EW_b1, a.EW_ln, a.EW_w2);
  __syncthreads();                                       // (before any wave leaves)
  const int N = a.NP + a.NL, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int centre = (int)blockIdx.x * 4 + w;
  if (centre >= a.B * N) return;
  const int b = centre / N, i = centre % N;
  const bool masked = a.nl_real != nullptr;
  const int npb = masked && a.np_real ? a.np_real[b] : a.NP, nlb = masked ? a.nl_real[b] : a.NL;
  if (masked && !atom_is_real(i, a.NP, npb, nlb)) {        // a padding atom is no centre: its list is never read
    if (lane < a.K) a.nbr[(long)centre * a.K + lane] = 0;
    return;
  }
  const PosView pv = pos_view(a, b);
  knn_wave<CAND>(pv, i, N, a.K, a.nbr + (long)centre * a.K, masked, npb, nlb, sel[w], srt[w]);
  ew_wave(pv, i, a.K, srt[w], a.EW_W1T, lw, a.EW_b2, a.ew + (long)centre * a.K);
}
// (a kernel of its own: the copy blocks need many waves per SIMD, the graph blocks ~200 registers per lane)
template <int PLW>
__global__ __launch_bounds__(256) void k_head_rows(const EmbedArgs e, const Layer0RowsArgs r) {
  const unsigned blk = blockIdx.x;
  if ((int)blk < e.blocks) embed_block(blk, e);
  else layer0_rows_block<PLW>(blk - e.blocks, r);
}

// --------------------------------------------------------------------------- bond-layer assemble
// For bond edge e = (src s -> dst t) of sample b (dst-major id e = t*(NL-1) + s'):
//   Ek[e] = PB.k_hb[e] + Wg1k . G(d_e) + PL[s].k_hk + PL[t].k_hj        (b1 folded into PB bias)
//   Ev[e] = same with the v weights
//   q1[e] = PB.q_hb[e] + PL[t].q_hi
// PB row layout [640]: NB ke | NB ve | BL k_hb | BL v_hb | BL q_hb;  PL row layout [1280]: see packing.py.
//   Rk[e] = Wg2k . G(d_e),  Rv[e] = Wg2v . G(d_e)   (the G(d_ji) columns, constant over a triplet segment)
// 16 bonds per wave tile, lane = (bond mm, channel group cg), 32 channels per lane as in
// the attention kernel's k-pass layout.  The four Gaussian contractions  out^T[c][bond] += sum_g W[g][c] G[bond][g]
// (20 Gaussians = 5 k-steps of v_mfma_f32_16x16x4_f32) take the tables as A operands from a channel-permuted LDS image
// (packing.py BL_Wgp, 40 KB) and the per-lane Gaussians as B; the gathered projection rows enter as the accumulator.
typedef float f32x4a __attribute__((ext_vector_type(4)));
//
// WIDE = false: the narrow bond layer (h_node_in_bond_net: False, uni_transformer_edge.py:147-152) -- its first Linears have no
// atom columns, so Ek / Ev start from PB.k_hb / PB.v_hb alone, PL is never read, and there is no fifth output block (the query
// MLP's hidden row is PB.q_hb as it stands).  Adding the wide model's atom rows when they are exact zeros changes no bit.
// (two waves per SIMD asked for: left alone, the compiler takes 216 VGPRs + 60 AGPRs = one wave per SIMD, i.e. ONE workgroup per
// CU and 2.1 rounds for the 545 workgroups of a C-small batch; -1.0 % step time, no spills, bit-identical)
template <bool WIDE>
__global__ __launch_bounds__(256, 2) void k_bl_assemble3(const float* __restrict__ x, const float* __restrict__ PB,
                                                      const float* __restrict__ PL, const float* __restrict__ Wgp /*[4,20,128]*/,
                                                      int B, int NP, int NL, float* __restrict__ Ek, float* __restrict__ Ev,
                                                      float* __restrict__ q1, float* __restrict__ Rk, float* __restrict__ Rv,
                                                      int blocks_per_output, const float* __restrict__ xprev,
                                                      const float* __restrict__ dxe, const float* __restrict__ dxb,
                                                      float* __restrict__ xout, const FlagWait fw) {
  // Deferred coordinate update (xprev != nullptr): the previous layer's x += dx_edge + dx_bond (uni_transformer_edge.py:285)
  // has not been applied yet -- every lane forms its two ligand positions from xprev + deltas (same association as
  // k_xupdate, so bit-identical) and workgroup 0 writes the updated rows for the kernels that follow.
  if (xprev != nullptr && blockIdx.x == 0) {
    const int n = B * NL * 3;
    for (int idx = threadIdx.x; idx < n; idx += 256) {
      const int bb = idx / (NL * 3), r = idx % (NL * 3);
      const long xi = ((long)bb * (NP + NL) + NP) * 3 + r;
      xout[xi] = xprev[xi] + dxe[idx] + dxb[idx];
    }
  }
  // workgroup = (output q: Ek, Ev, Rk, Rv, q1; four consecutive 16-bond tiles, one per wave): 5x the parallelism of a
  // tile-per-wave split over all outputs (only 435 tiles exist at B=8), and only that output's 10 KB table is staged
  __shared__ __attribute__((aligned(16))) float tab[DD_NGAUSS * 128];
  const int q = blockIdx.x / blocks_per_output;
  if (q < 4) {
    const float4* src = reinterpret_cast<const float4*>(Wgp + q * DD_NGAUSS * 128);
    for (int i = threadIdx.x; i < DD_NGAUSS * 32; i += 256) reinterpret_cast<float4*>(tab)[i] = src[i];
  }
  // PB / PL of this layer come from the layer-tail queue on the other stream: no graph edge, the counters are polled here
  // (the table above is staged meanwhile); ends with the barrier that also publishes the table
  if (fw.flags != nullptr) dd_wait_flags(fw.flags, fw.idx0, fw.n0, fw.idx1, fw.n1, DD_FLAG_ERR, 300);
  else __syncthreads();
  const int lane = threadIdx.x & 63, mm = lane & 15, cg = lane >> 4;
  const int Eb = NL * (NL - 1), N = NP + NL;
  const long nrows = (long)B * Eb;
  const long tile = (long)(blockIdx.x % blocks_per_output) * 4 + (threadIdx.x >> 6);
  if (tile * 16 >= nrows) return;
  const long e_raw = tile * 16 + mm;
  const bool valid = e_raw < nrows;
  const long e_glob = valid ? e_raw : nrows - 1;
  const int b = e_glob / Eb, e = e_glob % Eb;
  const int t = e / (NL - 1), sp = e % (NL - 1);
  const int s = sp + (sp >= t ? 1 : 0);
  const float* pb = PB + e_glob * 640 + 4 * cg;
  const float* ps = WIDE ? PL + ((long)b * NL + s) * 1280 + 4 * cg : nullptr;
  const float* pt = WIDE ? PL + ((long)b * NL + t) * 1280 + 4 * cg : nullptr;
  auto ld4 = [](const float* p) { return *reinterpret_cast<const float4*>(p); };
  if (WIDE && q == 4) {                                        // q1 = q_hb[e] + q_hi[t]
    if (q1 != nullptr && valid) {
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        const float4 a0 = ld4(pb + 512 + 16 * nt), a1 = ld4(pt + 1152 + 16 * nt);
        *reinterpret_cast<float4*>(q1 + e_glob * 128 + 4 * cg + 16 * nt) = make_float4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);
      }
    }
    return;
  }
  f32x4a acc[8];
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) {
    if (q < 2) {
      const float4 a0 = ld4(pb + 256 + 128 * q + 16 * nt);          // k_hb | v_hb
      if constexpr (WIDE) {
        const float4 a1 = ld4(ps + 640 + 256 * q + 16 * nt);        // k_hk | v_hk
        const float4 a2 = ld4(pt + 768 + 256 * q + 16 * nt);        // k_hj | v_hj
        acc[nt] = f32x4a{(a0.x + a1.x) + a2.x, (a0.y + a1.y) + a2.y, (a0.z + a1.z) + a2.z, (a0.w + a1.w) + a2.w};
      } else {
        acc[nt] = f32x4a{a0.x, a0.y, a0.z, a0.w};
      }
    } else {
      acc[nt] = f32x4a{0.f, 0.f, 0.f, 0.f};
    }
  }
  float dx, dy, dz;
  if (xprev != nullptr) {
    const float* xl = xprev + ((long)b * N + NP) * 3;
    const float* de = dxe + (long)b * NL * 3;
    const float* db = dxb + (long)b * NL * 3;
    dx = (xl[3 * t] + de[3 * t] + db[3 * t]) - (xl[3 * s] + de[3 * s] + db[3 * s]);
    dy = (xl[3 * t + 1] + de[3 * t + 1] + db[3 * t + 1]) - (xl[3 * s + 1] + de[3 * s + 1] + db[3 * s + 1]);
    dz = (xl[3 * t + 2] + de[3 * t + 2] + db[3 * t + 2]) - (xl[3 * s + 2] + de[3 * s + 2] + db[3 * s + 2]);
  } else {
    const float* xl = x + ((long)b * N + NP) * 3;
    dx = xl[3 * t] - xl[3 * s]; dy = xl[3 * t + 1] - xl[3 * s + 1]; dz = xl[3 * t + 2] - xl[3 * s + 2];
  }
  const float d = sqrtf(dx * dx + dy * dy + dz * dz);
  const float* tb = tab + cg * 128 + mm * 4;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float fk = gauss_feat(d, 4 * k + cg);
    const float4 w0 = *reinterpret_cast<const float4*>(tb + k * 512);
    const float4 w1 = *reinterpret_cast<const float4*>(tb + k * 512 + 64);
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.x, fk, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.y, fk, acc[1], 0, 0, 0);
    acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.z, fk, acc[2], 0, 0, 0);
    acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.w, fk, acc[3], 0, 0, 0);
    acc[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.x, fk, acc[4], 0, 0, 0);
    acc[5] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.y, fk, acc[5], 0, 0, 0);
    acc[6] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.z, fk, acc[6], 0, 0, 0);
    acc[7] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.w, fk, acc[7], 0, 0, 0);
  }
  float* dst = (q == 0 ? Ek : (q == 1 ? Ev : (q == 2 ? Rk : Rv))) + e_glob * 128 + 4 * cg;
  if (valid) {
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
      *reinterpret_cast<float4*>(dst + 16 * nt) = make_float4(acc[nt][0], acc[nt][1], acc[nt][2], acc[nt][3]);
  }
}

// x0-hat: ligand rows of the final coordinates
__global__ void k_extract_ligand(const float* __restrict__ x, int B, int NP, int NL, float* __restrict__ out) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * NL * 3) return;
  int b = idx / (NL * 3), r = idx % (NL * 3);
  out[idx] = x[((long)b * (NP + NL) + NP) * 3 + r];
}
int launch_extract_ligand(const float* x, int B, int NP, int NL, float* out, hipStream_t st) {
  int n = B * NL * 3;
  hipLaunchKernelGGL(k_extract_ligand, dim3((n + 255) / 256), dim3(256), 0, st, x, B, NP, NL, out);
  DD_CHECK_LAUNCH();
  return DD_OK;
}

// x_next[ligand rows] = x + dx_edge + dx_bond   (x = x + delta_x * mask_ligand, uni_transformer_edge.py:285)
__global__ void k_xupdate(const float* __restrict__ x, const float* __restrict__ dxe, const float* __restrict__ dxb,
                          int B, int NP, int NL, float* __restrict__ x_next) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * NL * 3) return;
  int b = idx / (NL * 3), r = idx % (NL * 3);
  long xi = ((long)b * (NP + NL) + NP) * 3 + r;
  x_next[xi] = x[xi] + dxe[idx] + dxb[idx];
}
int launch_xupdate(const float* x, const float* dxe, const float* dxb, int B, int NP, int NL, float* x_next, hipStream_t st) {
  int n = B * NL * 3;
  hipLaunchKernelGGL(k_xupdate, dim3((n + 255) / 256), dim3(256), 0, st, x, dxe, dxb, B, NP, NL, x_next);
  DD_CHECK_LAUNCH();
  return DD_OK;
}

// Candidates per lane are a template argument of the kNN kernels: calls f(std::integral_constant<int, C>) for the first
// class C of the list with cand <= C (the last one holds every supported size)
template <int C, int... Rest, class F>
static void with_cand_class(int cand, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, C>{});
  else if (cand <= C) f(std::integral_constant<int, C>{});
  else with_cand_class<Rest...>(cand, f);
}
static dim3 graph_grid(const GraphArgs& a) { return dim3((unsigned)((a.B * (a.NP + a.NL) + 3) / 4)); }   // one wave per centre

// (launch_knn / launch_edge_weights: one [B, N, 3] block only; shapes are checked by their callers, the op-level entry
// points and check_shapes)
static bool is_block(const GraphArgs& a) {
  return a.lig == a.prot + 3 * (long)a.NP && a.prot_stride == 3 * (a.NP + a.NL) && a.lig_stride == a.prot_stride;
}
int launch_knn(const GraphArgs& a, hipStream_t st) {
  if (!is_block(a)) return DD_ERR_BAD_ARG;
  with_cand_class<2, 4, 6, 11, 16, DD_N_MAX / 64>((a.NP + a.NL + 63) / 64, [&](auto c) {
    hipLaunchKernelGGL(k_knn<decltype(c)::value>, graph_grid(a), dim3(256), 0, st, a);
  });
  DD_CHECK_LAUNCH();
  return DD_OK;
}
int launch_edge_weights(const GraphArgs& a, hipStream_t st) {
  if (!is_block(a)) return DD_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_edge_weights2, graph_grid(a), dim3(256), 0, st, a);
  DD_CHECK_LAUNCH();
  return DD_OK;
}
int launch_graph(const GraphArgs& a, hipStream_t st) {
  const int N = a.NP + a.NL;
  if (!a.lig || (a.NP > 0 && !a.prot) || !a.nbr || !a.ew || a.B <= 0 || a.NP < 0 || a.NL <= 0) return DD_ERR_BAD_ARG;
  if (a.K <= 0 || a.K > DD_KNN_MAX || a.K > N - 1 || N > DD_N_MAX) return DD_ERR_UNSUPPORTED_SHAPE;
  with_cand_class<2, 4, 6, 11, 16, DD_N_MAX / 64>((N + 63) / 64, [&](auto c) {
    constexpr int CAND = decltype(c)::value;
    if (a.K <= 32) hipLaunchKernelGGL((k_graph<CAND, 32>), graph_grid(a), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_graph<CAND, 64>), graph_grid(a), dim3(256), 0, st, a);
  });
  DD_CHECK_LAUNCH();
  return DD_OK;
}
int launch_embed(const EmbedArgs& e, hipStream_t st) {
  hipLaunchKernelGGL(k_embed_all, dim3((unsigned)e.blocks), dim3(256), 0, st, e);
  DD_CHECK_LAUNCH();
  return DD_OK;
}
int launch_layer0_rows(const Layer0RowsArgs& r, hipStream_t st) {
  if (r.pl_width == 640) hipLaunchKernelGGL(k_layer0_rows<640>, dim3((unsigned)r.blocks), dim3(256), 0, st, r);
  else hipLaunchKernelGGL(k_layer0_rows<1280>, dim3((unsigned)r.blocks), dim3(256), 0, st, r);
  DD_CHECK_LAUNCH();
  return DD_OK;
}
int launch_head_rows(const EmbedArgs& e, const Layer0RowsArgs* r, hipStream_t st) {
  if (r != nullptr && e.nv != DD_NUM_V) return DD_ERR_UNSUPPORTED_SHAPE;   // (the tables hold DD_NUM_V classes x arm flag)
  const dim3 grid((unsigned)(e.blocks + (r ? r->blocks : 0)));
  if (r != nullptr && r->pl_width == 640) hipLaunchKernelGGL(k_head_rows<640>, grid, dim3(256), 0, st, e, *r);
  else hipLaunchKernelGGL(k_head_rows<1280>, grid, dim3(256), 0, st, e, r ? *r : Layer0RowsArgs{});
  DD_CHECK_LAUNCH();
  return DD_OK;
}
int launch_bl_assemble(const AssembleArgs& a, hipStream_t st) {
  if (a.Wgp == nullptr) return DD_ERR_BAD_ARG;
  const long rows = (long)a.B * a.NL * (a.NL - 1);
  const long tiles = (rows + 15) / 16;
  const int bpo = (int)((tiles + 3) / 4);                            // blocks per output (4 tiles each)
  if (a.narrow) {                                                    // (no atom rows, no q1 block)
    if (a.q1 != nullptr) return DD_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_bl_assemble3<false>, dim3((unsigned)(bpo * 4)), dim3(256), 0, st, a.x, a.PB, nullptr, a.Wgp, a.B, a.NP, a.NL,
                       a.Ek, a.Ev, nullptr, a.Rk, a.Rv, bpo, a.xprev, a.dxe, a.dxb, a.xout, a.fw);
  } else {
    hipLaunchKernelGGL(k_bl_assemble3<true>, dim3((unsigned)(bpo * (a.q1 ? 5 : 4))), dim3(256), 0, st, a.x, a.PB, a.PL, a.Wgp, a.B, a.NP,
                       a.NL, a.Ek, a.Ev, a.q1, a.Rk, a.Rv, bpo, a.xprev, a.dxe, a.dxb, a.xout, a.fw);
  }
  DD_CHECK_LAUNCH();
  return DD_OK;
}

}  // namespace dd

// Op-level graph entry points: a [B, N, 3] tensor is a problem of N "protein" rows (no ligand block, no padding)
static dd::GraphArgs graph_args(const float* x, int B, int NP, int NL, int K, int32_t* nbr) {
  dd::GraphArgs a{};
  a.B = B; a.NP = NP; a.NL = NL; a.K = K; a.nbr = nbr;
  a.set_block(x);
  return a;
}
extern "C" int dd_knn(const float* x, int B, int N, int K, int32_t* nbr, void* stream) {
  if (!x || !nbr || B <= 0 || N <= 1) return DD_ERR_BAD_ARG;
  if (N > DD_N_MAX || K > DD_KNN_MAX || K > N - 1 || K <= 0) return DD_ERR_UNSUPPORTED_SHAPE;
  return dd::launch_knn(graph_args(x, B, N, 0, K, nbr), (hipStream_t)stream);
}

// ... for a padded heterogeneous batch (the sampler's layout: NP + NL rows per sample, the real atoms are the first np_real[b]
// protein rows and the first nl_real[b] ligand rows): padding atoms are neither centres nor candidates.
extern "C" int dd_knn_masked(const float* x, int B, int NP, int NL, int K, const int32_t* np_real, const int32_t* nl_real, int32_t* nbr,
                             void* stream) {
  const int N = NP + NL;
  if (!x || !nbr || !nl_real || B <= 0 || NP < 0 || NL <= 0 || K <= 0 || K > DD_KNN_MAX || K > N - 1 || N > DD_N_MAX) return DD_ERR_BAD_ARG;
  dd::GraphArgs a = graph_args(x, B, NP, NL, K, nbr);
  a.np_real = np_real; a.nl_real = nl_real;
  return dd::launch_knn(a, (hipStream_t)stream);
}

// ... for a flat PyG batch of different samples (k_knn_csr).  n_max (the largest sample) only picks the chunk size: the
// candidates are streamed, so every value gives the same result.
extern "C" int dd_knn_csr(const float* x, const int32_t* ptr, int B, int n, int n_max, int K, int loop, const int64_t* out_off,
                          int64_t E, int64_t* edge_index, void* stream) {
  if (!ptr || !out_off || B <= 0 || n < 0 || E < 0 || K <= 0 || (loop != 0 && loop != 1)) return DD_ERR_BAD_ARG;
  if (K > DD_KNN_MAX) return DD_ERR_UNSUPPORTED_SHAPE;
  if (n == 0 || E == 0) return DD_OK;
  if (!x || !edge_index) return DD_ERR_BAD_ARG;
  const dim3 grid((unsigned)(((long)n + 3) / 4)), block(256);
  dd::with_cand_class<2, 4, 8, 16, DD_N_MAX / 64>((n_max + 63) / 64, [&](auto c) {
    hipLaunchKernelGGL(dd::k_knn_csr<decltype(c)::value>, grid, block, 0, (hipStream_t)stream, x, ptr, B, n, K, loop, out_off, (long)E,
                       edge_index);
  });
  DD_CHECK_LAUNCH();
  return DD_OK;
}

extern "C" int dd_edge_weights(const float* x, const int32_t* nbr, int B, int N, int K, const float* W1T,
                               const float* b1, const float* ln, const float* w2, const float* b2, float* ew,
                               void* stream) {
  if (!x || !nbr || !W1T || !b1 || !ln || !w2 || !b2 || !ew) return DD_ERR_BAD_ARG;
  dd::GraphArgs a = graph_args(x, B, N, 0, K, const_cast<int32_t*>(nbr));   // (the list is only read here)
  a.ew = ew; a.EW_W1T = W1T; a.EW_b1 = b1; a.EW_ln = ln; a.EW_w2 = w2; a.EW_b2 = b2;
  return dd::launch_edge_weights(a, (hipStream_t)stream);
}

extern "C" int dd_embed_protein(const float* protein_v, int rows, const float* W, const float* b, float* protein_h,
                                void* stream) {
  if (!protein_v || !W || !b || !protein_h || rows <= 0) return DD_ERR_BAD_ARG;
  long n = (long)rows * 128;
  hipLaunchKernelGGL(dd::k_embed_protein, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     protein_v, rows, W, b, protein_h);
  DD_CHECK_LAUNCH();
  return DD_OK;
}
