// Op-level message passing: the torch_scatter call pairs of the reference as stand-alone kernels (SURVEY.md 8b,
// "op-level boundary").  The sampling loop itself runs the fused kernels of dd_attention2.hip, where q / k / v never
// touch HBM; these are for hosts that keep the reference's Python layers and only swap
//
//     alpha = scatter_softmax((q[dst] * k / sqrt(d)).sum(-1), dst, dim=0)
//     out   = scatter_sum(alpha.unsqueeze(-1) * v, dst, dim=0, dim_size=N)
//
// (models/encoders/uni_transformer_edge.py:63-68 node, :158-164 triplet, :205-211 coordinates), and they are the kernels the
// HBM roofline of SURVEY.md 8d(i) is quoted on: every byte of q, k, v, e_w and the segment pointers is read once, the
// output written once.
//
// Edges must be grouped by destination (knn_graph, the dst-major bond list and the SparseTensor triplets all are):
// seg_ptr[s] .. seg_ptr[s+1] are the edges of destination s.  One wavefront owns one destination; lane l holds
// channels 2l, 2l+1 (head l / 4), so a k or v row is one 512-byte wave load.  Softmax is the single-pass form
// (running maximum, rescaled running sum) in edge order; 4 edges are in flight per wave.
//
// The bodies attn_aggregate<POS, MASK> and attn_aggregate_bwd<POS, MASK> (POS: the coordinate form; MASK: the member masks of
// padded batches, below) sit behind four thin kernels per direction pair -- k_attn_aggregate<POS>, k_attn_aggregate_masked<POS> and
// their _bwd forms; the unmasked ones take no mask argument.  One host launcher per direction, launch_attn_aggregate<POS> and
// launch_attn_aggregate_bwd<POS>, holds the argument check, the grid and the launch: the nine exported dd_attn_aggregate_* entry
// points forward to these, and a NULL member_mask launches the unmasked kernel.
#include "dd_common.hpp"
#include "dd_kernels.hpp"

namespace dd {

namespace {

constexpr int UNROLL = 4;

// sum over the 4 lanes of a head (lanes 4h .. 4h+3)
__device__ __forceinline__ float head_sum(float v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  return v;
}

// Member masks (MASK; padded batches): member_mask[e] != 0 means member e is real.  A masked member does not exist: its byte is
// wave-uniform, and a scalar branch steps over everything that would use its k / v / e_w / rel_x (and per-edge q) rows, so
// whatever those rows hold -- NaN included -- reaches no result.  The real members run through the same recurrence, in member
// order, with the same expressions: the results are bit for bit those of the segment compacted to its real members.

// first real member of the segment e0 .. e1, or -1 (wave-uniform): 64 mask bytes per ballot
__device__ __forceinline__ int first_real(const uint8_t* __restrict__ member_mask, int e0, int e1, int lane) {
  for (int b = e0; b < e1; b += 64) {
    const int ee = b + lane;
    const unsigned long long real = __ballot(ee < e1 && member_mask[ee] != 0);
    if (real) return __builtin_amdgcn_readfirstlane(b + __ffsll(real) - 1);
  }
  return -1;
}

template <bool POS, bool MASK>
__device__ __forceinline__ void attn_aggregate(const float* __restrict__ q, int q_per_edge, const float* __restrict__ k,
                                               const float* __restrict__ v, const float* __restrict__ e_w,
                                               const float* __restrict__ rel_x, const int32_t* __restrict__ seg_ptr,
                                               const uint8_t* __restrict__ member_mask, int n_seg, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  // the segment and its edge range are wave-uniform: kept in SGPRs, so e_w / rel_x / seg_ptr become scalar loads
  const int seg = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (seg >= n_seg) return;
  const int e0 = __builtin_amdgcn_readfirstlane(seg_ptr[seg]), e1 = __builtin_amdgcn_readfirstlane(seg_ptr[seg + 1]);
  const int ef = MASK ? first_real(member_mask, e0, e1, lane) : e0;                // (per-edge q is read from this member's row)
  if (e1 <= e0 || (MASK && ef < 0)) {                    // scatter_sum leaves untouched rows at zero
    if (POS) { if (lane < 3) out[(long)seg * 3 + lane] = 0.f; }
    else *reinterpret_cast<float2*>(out + (long)seg * 128 + 2 * lane) = make_float2(0.f, 0.f);
    return;
  }
  const float2 qv = *reinterpret_cast<const float2*>(q + (long)(q_per_edge ? ef : seg) * 128 + 2 * lane);
  const float scale = 0.35355339059327373f;              // 1 / sqrt(8)
  float mx = -INFINITY, den = 0.f;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;                    // !POS: a0, a1 = channels 2l, 2l+1; POS: xyz of head l/4
  const int head = lane >> 2;
  for (int e = e0; e < e1; e += UNROLL) {
    float2 kk[UNROLL], vv[UNROLL];
    float w[UNROLL], r[UNROLL][3];
    int real[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long ee = e + u < e1 ? e + u : e1 - 1;       // clamped: the tail replays the last edge and is masked below
      real[u] = MASK ? __builtin_amdgcn_readfirstlane(member_mask[ee]) : 1;
      kk[u] = *reinterpret_cast<const float2*>(k + ee * 128 + 2 * lane);
      if (POS) {
        vv[u].x = v[ee * 16 + head];
        r[u][0] = rel_x[ee * 3]; r[u][1] = rel_x[ee * 3 + 1]; r[u][2] = rel_x[ee * 3 + 2];
      } else {
        vv[u] = *reinterpret_cast<const float2*>(v + ee * 128 + 2 * lane);
      }
      w[u] = e_w ? e_w[ee] : 1.0f;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (e + u >= e1) break;
      if (MASK && !real[u]) continue;
      const float s = head_sum(fmaf(qv.y, kk[u].y, qv.x * kk[u].x)) * scale;
      const float mn = fmaxf(mx, s);
      const float corr = __expf(mx - mn), p = __expf(s - mn);    // (mx = -inf on the first edge: corr = 0)
      den = fmaf(den, corr, p);
      if (POS) {
        const float pv = p * (vv[u].x * w[u]);
        a0 = fmaf(a0, corr, pv * r[u][0]); a1 = fmaf(a1, corr, pv * r[u][1]); a2 = fmaf(a2, corr, pv * r[u][2]);
      } else {
        a0 = fmaf(a0, corr, p * (vv[u].x * w[u])); a1 = fmaf(a1, corr, p * (vv[u].y * w[u]));
      }
      mx = mn;
    }
  }
  const float inv = 1.0f / den;
  if (POS) {
    // mean over the 16 heads: one lane per head carries the head's vector
    const bool lead = (lane & 3) == 0;
    const float x = wave_sum(lead ? a0 * inv : 0.f), y = wave_sum(lead ? a1 * inv : 0.f), z = wave_sum(lead ? a2 * inv : 0.f);
    if (lane == 0) { out[(long)seg * 3] = x * 0.0625f; out[(long)seg * 3 + 1] = y * 0.0625f; out[(long)seg * 3 + 2] = z * 0.0625f; }
  } else {
    *reinterpret_cast<float2*>(out + (long)seg * 128 + 2 * lane) = make_float2(a0 * inv, a1 * inv);
  }
}

template <bool POS>
__global__ __launch_bounds__(256) void k_attn_aggregate(const float* __restrict__ q, int q_per_edge, const float* __restrict__ k,
                                                        const float* __restrict__ v, const float* __restrict__ e_w,
                                                        const float* __restrict__ rel_x, const int32_t* __restrict__ seg_ptr,
                                                        int n_seg, float* __restrict__ out) {
  attn_aggregate<POS, false>(q, q_per_edge, k, v, e_w, rel_x, seg_ptr, nullptr, n_seg, out);
}

template <bool POS>
__global__ __launch_bounds__(256) void k_attn_aggregate_masked(const float* __restrict__ q, int q_per_edge, const float* __restrict__ k,
                                                               const float* __restrict__ v, const float* __restrict__ e_w,
                                                               const float* __restrict__ rel_x, const int32_t* __restrict__ seg_ptr,
                                                               const uint8_t* __restrict__ member_mask, int n_seg,
                                                               float* __restrict__ out) {
  attn_aggregate<POS, true>(q, q_per_edge, k, v, e_w, rel_x, seg_ptr, member_mask, n_seg, out);
}

// ---- backward of k_attn_aggregate, same mapping (a wave per destination, lane l = channels 2l, 2l+1, 4 members in flight).
// With g = d_out, alpha = the forward's softmax weight, w = e_w (1 without), per member e and head h:
//   node form:        t = w * sum_{c in h} g[s,c] v[e,c]          D = sum_{c in h} g[s,c] out[s,c]   (= sum_e alpha t)
//   coordinate form:  t = w * v16[e,h] * (g[s] . rel[e]) / 16     D = sum_e alpha t
//   ds = alpha (t - D);   dk[e] = scale ds q[s];   dq[s] = scale sum_e ds k[e]   (q per edge: dq[e] = scale ds k[e])
// Nothing is saved by the forward: pass 1 reads the segment's k rows (coordinate form: v16, rel_x, e_w too, for D) and forms
// the running maximum and denominator as the forward does, pass 2 reads the members again, forms alpha and writes every
// gradient.  No atomics: each output element is written by one lane, once -- reproducible bit for bit, and the buffers
// need no initialisation.  An empty segment writes its zero dq row (q per segment) and nothing else.
// MASK: a masked member takes no part in either pass and gets zeros in its dk, dv, d_ew, d_rel (and per-edge dq) rows -- still
// one write per element; a segment whose members are all masked does that for every member and writes its zero dq row.
// the gradient rows of a member that does not exist (MASK)
template <bool POS>
__device__ __forceinline__ void zero_member(long ee, int lane, int q_per_edge, float* __restrict__ dq, float* __restrict__ dk,
                                            float* __restrict__ dv, float* __restrict__ d_ew, float* __restrict__ d_rel) {
  const float2 z = make_float2(0.f, 0.f);
  *reinterpret_cast<float2*>(dk + ee * 128 + 2 * lane) = z;
  if (q_per_edge) *reinterpret_cast<float2*>(dq + ee * 128 + 2 * lane) = z;
  if (POS) {
    if ((lane & 3) == 0) dv[ee * 16 + (lane >> 2)] = 0.f;
    if (lane < 3) d_rel[ee * 3 + lane] = 0.f;
  } else {
    *reinterpret_cast<float2*>(dv + ee * 128 + 2 * lane) = z;
  }
  if (d_ew && lane == 0) d_ew[ee] = 0.f;
}

template <bool POS, bool MASK>
__device__ __forceinline__ void attn_aggregate_bwd(const float* __restrict__ q, int q_per_edge, const float* __restrict__ k,
                                                   const float* __restrict__ v, const float* __restrict__ e_w,
                                                   const float* __restrict__ rel_x, const int32_t* __restrict__ seg_ptr,
                                                   const uint8_t* __restrict__ member_mask, int n_seg, const float* __restrict__ out,
                                                   const float* __restrict__ d_out, float* __restrict__ dq, float* __restrict__ dk,
                                                   float* __restrict__ dv, float* __restrict__ d_ew, float* __restrict__ d_rel) {
  const int lane = threadIdx.x & 63;
  const int seg = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (seg >= n_seg) return;
  const int e0 = __builtin_amdgcn_readfirstlane(seg_ptr[seg]), e1 = __builtin_amdgcn_readfirstlane(seg_ptr[seg + 1]);
  if (e1 <= e0) {
    if (!q_per_edge) *reinterpret_cast<float2*>(dq + (long)seg * 128 + 2 * lane) = make_float2(0.f, 0.f);
    return;
  }
  const int ef = MASK ? first_real(member_mask, e0, e1, lane) : e0;
  if (MASK && ef < 0) {
    for (int e = e0; e < e1; ++e) zero_member<POS>(e, lane, q_per_edge, dq, dk, dv, d_ew, d_rel);
    if (!q_per_edge) *reinterpret_cast<float2*>(dq + (long)seg * 128 + 2 * lane) = make_float2(0.f, 0.f);
    return;
  }
  const float2 qv = *reinterpret_cast<const float2*>(q + (long)(q_per_edge ? ef : seg) * 128 + 2 * lane);
  const float scale = 0.35355339059327373f;              // 1 / sqrt(8)
  const int head = lane >> 2;
  const bool lead = (lane & 3) == 0;
  float2 gc = make_float2(0.f, 0.f);                     // !POS: g[s, 2l], g[s, 2l+1]
  float g0 = 0.f, g1 = 0.f, g2 = 0.f, gl = 0.f;          // POS: g[s, 0..2] (wave-uniform) and g[s, lane] on lanes 0..2
  if (POS) {
    g0 = d_out[(long)seg * 3]; g1 = d_out[(long)seg * 3 + 1]; g2 = d_out[(long)seg * 3 + 2];
    gl = lane == 0 ? g0 : (lane == 1 ? g1 : (lane == 2 ? g2 : 0.f));
  } else {
    gc = *reinterpret_cast<const float2*>(d_out + (long)seg * 128 + 2 * lane);
  }
  // ---- pass 1: running maximum and denominator in the forward's order (POS: D rides along)
  float mx = -INFINITY, den = 0.f, dacc = 0.f;
  for (int e = e0; e < e1; e += UNROLL) {
    float2 kk[UNROLL];
    float t[UNROLL];
    int real[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long ee = e + u < e1 ? e + u : e1 - 1;       // clamped, masked below
      real[u] = MASK ? __builtin_amdgcn_readfirstlane(member_mask[ee]) : 1;
      kk[u] = *reinterpret_cast<const float2*>(k + ee * 128 + 2 * lane);
      if (POS) {
        const float ue = fmaf(g0, rel_x[ee * 3], fmaf(g1, rel_x[ee * 3 + 1], g2 * rel_x[ee * 3 + 2])) * 0.0625f;
        t[u] = (v[ee * 16 + head] * (e_w ? e_w[ee] : 1.0f)) * ue;
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (e + u >= e1) break;
      if (MASK && !real[u]) continue;
      const float s = head_sum(fmaf(qv.y, kk[u].y, qv.x * kk[u].x)) * scale;
      const float mn = fmaxf(mx, s);
      const float corr = __expf(mx - mn), p = __expf(s - mn);
      den = fmaf(den, corr, p);
      if (POS) dacc = fmaf(dacc, corr, p * t[u]);
      mx = mn;
    }
  }
  const float inv = 1.0f / den;
  float D;
  if (POS) {
    D = dacc * inv;
  } else {
    const float2 ov = *reinterpret_cast<const float2*>(out + (long)seg * 128 + 2 * lane);
    D = head_sum(fmaf(gc.y, ov.y, gc.x * ov.x));
  }
  // ---- pass 2: alpha and every gradient (the k rows of the segment come from cache)
  float aq0 = 0.f, aq1 = 0.f;
  for (int e = e0; e < e1; e += UNROLL) {
    float2 kk[UNROLL], vv[UNROLL];
    float w[UNROLL], ue[UNROLL];
    int real[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long ee = e + u < e1 ? e + u : e1 - 1;       // clamped: nothing is stored for a replayed member
      real[u] = MASK ? __builtin_amdgcn_readfirstlane(member_mask[ee]) : 1;
      kk[u] = *reinterpret_cast<const float2*>(k + ee * 128 + 2 * lane);
      if (POS) {
        vv[u].x = v[ee * 16 + head];
        ue[u] = fmaf(g0, rel_x[ee * 3], fmaf(g1, rel_x[ee * 3 + 1], g2 * rel_x[ee * 3 + 2])) * 0.0625f;
      } else {
        vv[u] = *reinterpret_cast<const float2*>(v + ee * 128 + 2 * lane);
      }
      w[u] = e_w ? e_w[ee] : 1.0f;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (e + u >= e1) break;
      const long ee = e + u;
      if (MASK && !real[u]) { zero_member<POS>(ee, lane, q_per_edge, dq, dk, dv, d_ew, d_rel); continue; }
      const float s = head_sum(fmaf(qv.y, kk[u].y, qv.x * kk[u].x)) * scale;
      const float a = __expf(s - mx) * inv;
      float ds;
      if (POS) {
        ds = a * ((vv[u].x * w[u]) * ue[u] - D);
        const float av = wave_sum(lead ? a * vv[u].x : 0.f);                   // sum_h alpha v16
        if (lead) dv[ee * 16 + head] = a * w[u] * ue[u];
        if (d_ew && lane == 0) d_ew[ee] = ue[u] * av;
        if (lane < 3) d_rel[ee * 3 + lane] = gl * (w[u] * 0.0625f) * av;
      } else {
        const float gv = head_sum(fmaf(gc.y, vv[u].y, gc.x * vv[u].x));
        ds = a * (w[u] * gv - D);
        const float aw = a * w[u];
        *reinterpret_cast<float2*>(dv + ee * 128 + 2 * lane) = make_float2(aw * gc.x, aw * gc.y);
        if (d_ew) {
          const float x = wave_sum(lead ? a * gv : 0.f);
          if (lane == 0) d_ew[ee] = x;
        }
      }
      const float dsq = ds * scale;
      *reinterpret_cast<float2*>(dk + ee * 128 + 2 * lane) = make_float2(dsq * qv.x, dsq * qv.y);
      if (q_per_edge) {
        *reinterpret_cast<float2*>(dq + ee * 128 + 2 * lane) = make_float2(dsq * kk[u].x, dsq * kk[u].y);
      } else {
        aq0 = fmaf(dsq, kk[u].x, aq0); aq1 = fmaf(dsq, kk[u].y, aq1);
      }
    }
  }
  if (!q_per_edge) *reinterpret_cast<float2*>(dq + (long)seg * 128 + 2 * lane) = make_float2(aq0, aq1);
}

template <bool POS>
__global__ __launch_bounds__(256) void k_attn_aggregate_bwd(const float* __restrict__ q, int q_per_edge, const float* __restrict__ k,
                                                            const float* __restrict__ v, const float* __restrict__ e_w,
                                                            const float* __restrict__ rel_x, const int32_t* __restrict__ seg_ptr,
                                                            int n_seg, const float* __restrict__ out, const float* __restrict__ d_out,
                                                            float* __restrict__ dq, float* __restrict__ dk, float* __restrict__ dv,
                                                            float* __restrict__ d_ew, float* __restrict__ d_rel) {
  attn_aggregate_bwd<POS, false>(q, q_per_edge, k, v, e_w, rel_x, seg_ptr, nullptr, n_seg, out, d_out, dq, dk, dv, d_ew, d_rel);
}

template <bool POS>
__global__ __launch_bounds__(256) void k_attn_aggregate_bwd_masked(const float* __restrict__ q, int q_per_edge, const float* __restrict__ k,
                                                                   const float* __restrict__ v, const float* __restrict__ e_w,
                                                                   const float* __restrict__ rel_x, const int32_t* __restrict__ seg_ptr,
                                                                   const uint8_t* __restrict__ member_mask, int n_seg,
                                                                   const float* __restrict__ out, const float* __restrict__ d_out,
                                                                   float* __restrict__ dq, float* __restrict__ dk, float* __restrict__ dv,
                                                                   float* __restrict__ d_ew, float* __restrict__ d_rel) {
  attn_aggregate_bwd<POS, true>(q, q_per_edge, k, v, e_w, rel_x, seg_ptr, member_mask, n_seg, out, d_out, dq, dk, dv, d_ew, d_rel);
}

// ---- host side: the argument check of the node (!POS) or coordinate (POS) entry points, and the masked or the unmasked
// kernel by member_mask != NULL (NULL: all members are real -- the unmasked kernel, which has no mask argument)
template <bool POS>
int launch_attn_aggregate(const float* q, int q_per_edge, const float* k, const float* v, const float* e_w, const float* rel_x,
                          const int32_t* seg_ptr, int n_seg, const uint8_t* member_mask, float* out, void* stream) {
  if (!q || !k || !v || (POS && !rel_x) || !seg_ptr || !out || n_seg < 0) return DD_ERR_BAD_ARG;
  if (n_seg == 0) return DD_OK;
  const dim3 grid((n_seg + 3) / 4), block(256);
  if (member_mask)
    hipLaunchKernelGGL(k_attn_aggregate_masked<POS>, grid, block, 0, (hipStream_t)stream, q, q_per_edge, k, v, e_w, rel_x, seg_ptr,
                       member_mask, n_seg, out);
  else
    hipLaunchKernelGGL(k_attn_aggregate<POS>, grid, block, 0, (hipStream_t)stream, q, q_per_edge, k, v, e_w, rel_x, seg_ptr, n_seg, out);
  DD_CHECK_LAUNCH();
  return DD_OK;
}

// (the node form reads `out` and has no rel_x / d_rel; the coordinate form recomputes D and has no `out`)
template <bool POS>
int launch_attn_aggregate_bwd(const float* q, int q_per_edge, const float* k, const float* v, const float* e_w, const float* rel_x,
                              const int32_t* seg_ptr, int n_seg, const uint8_t* member_mask, const float* out, const float* d_out,
                              float* dq, float* dk, float* dv, float* d_ew, float* d_rel, void* stream) {
  if (!q || !k || !v || (POS ? !rel_x || !d_rel : !out) || !seg_ptr || !d_out || !dq || !dk || !dv ||
      (e_w == nullptr) != (d_ew == nullptr) || n_seg < 0)
    return DD_ERR_BAD_ARG;
  if (n_seg == 0) return DD_OK;
  const dim3 grid((n_seg + 3) / 4), block(256);
  if (member_mask)
    hipLaunchKernelGGL(k_attn_aggregate_bwd_masked<POS>, grid, block, 0, (hipStream_t)stream, q, q_per_edge, k, v, e_w, rel_x, seg_ptr,
                       member_mask, n_seg, out, d_out, dq, dk, dv, d_ew, d_rel);
  else
    hipLaunchKernelGGL(k_attn_aggregate_bwd<POS>, grid, block, 0, (hipStream_t)stream, q, q_per_edge, k, v, e_w, rel_x, seg_ptr, n_seg, out,
                       d_out, dq, dk, dv, d_ew, d_rel);
  DD_CHECK_LAUNCH();
  return DD_OK;
}

// ---- stand-alone torch_scatter drop-ins: scatter_sum / scatter_mean / scatter_min / scatter_max and
// scatter_softmax over dim 0 of a [E, F] fp32 tensor whose rows are grouped by destination (CSR segments).  Call sites in
// the reference: scatter_softmax / scatter_sum in the three attention layers (uni_transformer_edge.py:64,68,160,164,205,209),
// scatter_mean in center_pos (decompdiff.py:25), scatter_min in the arm-scaffold drift (guidance_funcs.py:52).
// One wavefront per (segment, 64-feature chunk).  F <= 32: the wave also splits the segment's rows over 64 / Fp lane
// groups (Fp = F rounded up to a power of two), combined at the end in a fixed butterfly order -> deterministic.
enum { OP_SUM = 0, OP_MEAN = 1, OP_MIN = 2, OP_MAX = 3 };

__device__ __forceinline__ int seg_fp(int F) { int p = 1; while (p < F && p < 64) p <<= 1; return p; }

template <int OP>
__global__ __launch_bounds__(256) void k_segment_reduce(const float* __restrict__ src, const int32_t* __restrict__ seg_ptr, int n_seg,
                                                        int F, int n_chunk, float* __restrict__ out, int64_t* __restrict__ arg_out,
                                                        long E) {
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (long)n_seg * n_chunk) return;
  const int seg = (int)(w / n_chunk), chunk = (int)(w % n_chunk);
  const int e0 = seg_ptr[seg], e1 = seg_ptr[seg + 1];
  const int Fp = seg_fp(F), G = 64 / Fp;
  const int f = chunk * 64 + (lane & (Fp - 1)), g = lane / Fp;
  const bool fv = f < F;
  float acc = OP == OP_MIN ? INFINITY : (OP == OP_MAX ? -INFINITY : 0.f);
  long arg = E;
  for (int e = e0 + g; e < e1; e += G) {
    const float v = fv ? src[(long)e * F + f] : 0.f;
    if (OP == OP_MIN) { if (v < acc) { acc = v; arg = e; } }
    else if (OP == OP_MAX) { if (v > acc) { acc = v; arg = e; } }
    else acc += v;
  }
  for (int off = Fp; off < 64; off <<= 1) {              // combine the lane groups (ties: the smaller row index wins)
    const float o = __shfl_xor(acc, off);
    const long oa = __shfl_xor(arg, off);
    if (OP == OP_MIN) { if (o < acc || (o == acc && oa < arg)) { acc = o; arg = oa; } }
    else if (OP == OP_MAX) { if (o > acc || (o == acc && oa < arg)) { acc = o; arg = oa; } }
    else acc += o;
  }
  if (!fv || g != 0) return;
  if (e1 <= e0) { acc = 0.f; arg = E; }                  // torch_scatter: untouched rows are 0, their arg = src.size(dim)
  if (OP == OP_MEAN && e1 > e0) acc /= (float)(e1 - e0);
  out[(long)seg * F + f] = acc;
  if ((OP == OP_MIN || OP == OP_MAX) && arg_out) arg_out[(long)seg * F + f] = arg;
}

__global__ __launch_bounds__(256) void k_segment_softmax(const float* __restrict__ src, const int32_t* __restrict__ seg_ptr, int n_seg,
                                                         int F, int n_chunk, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (long)n_seg * n_chunk) return;
  const int seg = (int)(w / n_chunk), chunk = (int)(w % n_chunk);
  const int e0 = seg_ptr[seg], e1 = seg_ptr[seg + 1];
  const int Fp = seg_fp(F), G = 64 / Fp;
  const int f = chunk * 64 + (lane & (Fp - 1)), g = lane / Fp;
  const bool fv = f < F;
  float mx = -INFINITY;
  for (int e = e0 + g; e < e1; e += G) mx = fmaxf(mx, fv ? src[(long)e * F + f] : 0.f);
  for (int off = Fp; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  float sum = 0.f;
  for (int e = e0 + g; e < e1; e += G) sum += fv ? expf(src[(long)e * F + f] - mx) : 0.f;
  for (int off = Fp; off < 64; off <<= 1) sum += __shfl_xor(sum, off);
  if (!fv) return;
  for (int e = e0 + g; e < e1; e += G) out[(long)e * F + f] = expf(src[(long)e * F + f] - mx) / sum;
}

}  // namespace

}  // namespace dd

// ---- the attention entry points: member_mask [E], non-zero = the member is real; NULL (and every unmasked form) = all real
extern "C" int dd_attn_aggregate_node_masked(const float* q, int q_per_edge, const float* k, const float* v, const float* e_w,
                                             const int32_t* seg_ptr, int n_seg, const uint8_t* member_mask, float* out, void* stream) {
  return dd::launch_attn_aggregate<false>(q, q_per_edge, k, v, e_w, nullptr, seg_ptr, n_seg, member_mask, out, stream);
}

extern "C" int dd_attn_aggregate_pos_masked(const float* q, const float* k, const float* v16, const float* e_w, const float* rel_x,
                                            const int32_t* seg_ptr, int n_seg, const uint8_t* member_mask, float* out, void* stream) {
  return dd::launch_attn_aggregate<true>(q, 0, k, v16, e_w, rel_x, seg_ptr, n_seg, member_mask, out, stream);
}

extern "C" int dd_attn_aggregate_node_bwd_masked(const float* q, int q_per_edge, const float* k, const float* v, const float* e_w,
                                                 const int32_t* seg_ptr, int n_seg, const uint8_t* member_mask, const float* out,
                                                 const float* d_out, float* dq, float* dk, float* dv, float* d_ew, void* stream) {
  return dd::launch_attn_aggregate_bwd<false>(q, q_per_edge, k, v, e_w, nullptr, seg_ptr, n_seg, member_mask, out, d_out, dq, dk, dv, d_ew,
                                              nullptr, stream);
}

extern "C" int dd_attn_aggregate_pos_bwd_masked(const float* q, const float* k, const float* v16, const float* e_w, const float* rel_x,
                                                const int32_t* seg_ptr, int n_seg, const uint8_t* member_mask, const float* d_out,
                                                float* dq, float* dk, float* dv16, float* d_ew, float* d_rel, void* stream) {
  return dd::launch_attn_aggregate_bwd<true>(q, 0, k, v16, e_w, rel_x, seg_ptr, n_seg, member_mask, nullptr, d_out, dq, dk, dv16, d_ew,
                                             d_rel, stream);
}

extern "C" int dd_attn_aggregate_node(const float* q, int q_per_edge, const float* k, const float* v, const float* e_w,
                                      const int32_t* seg_ptr, int n_seg, float* out, void* stream) {
  return dd_attn_aggregate_node_masked(q, q_per_edge, k, v, e_w, seg_ptr, n_seg, nullptr, out, stream);
}

extern "C" int dd_attn_aggregate_triplet(const float* q, const float* k, const float* v, const int32_t* seg_ptr, int n_seg,
                                         float* out, void* stream) {
  return dd_attn_aggregate_node_masked(q, 1, k, v, nullptr, seg_ptr, n_seg, nullptr, out, stream);
}

extern "C" int dd_attn_aggregate_pos(const float* q, const float* k, const float* v16, const float* e_w, const float* rel_x,
                                     const int32_t* seg_ptr, int n_seg, float* out, void* stream) {
  return dd_attn_aggregate_pos_masked(q, k, v16, e_w, rel_x, seg_ptr, n_seg, nullptr, out, stream);
}

extern "C" int dd_attn_aggregate_node_bwd(const float* q, int q_per_edge, const float* k, const float* v, const float* e_w,
                                          const int32_t* seg_ptr, int n_seg, const float* out, const float* d_out, float* dq,
                                          float* dk, float* dv, float* d_ew, void* stream) {
  return dd_attn_aggregate_node_bwd_masked(q, q_per_edge, k, v, e_w, seg_ptr, n_seg, nullptr, out, d_out, dq, dk, dv, d_ew, stream);
}

extern "C" int dd_attn_aggregate_pos_bwd(const float* q, const float* k, const float* v16, const float* e_w, const float* rel_x,
                                         const int32_t* seg_ptr, int n_seg, const float* d_out, float* dq, float* dk, float* dv16,
                                         float* d_ew, float* d_rel, void* stream) {
  return dd_attn_aggregate_pos_bwd_masked(q, k, v16, e_w, rel_x, seg_ptr, n_seg, nullptr, d_out, dq, dk, dv16, d_ew, d_rel, stream);
}

extern "C" int dd_segment_reduce(const float* src, const int32_t* seg_ptr, int n_seg, int F, int op, long E, float* out,
                                 int64_t* arg_out, void* stream) {
  if (!seg_ptr || !out || n_seg < 0 || F <= 0 || E < 0 || (E > 0 && !src) || op < 0 || op > 3) return DD_ERR_BAD_ARG;
  if (n_seg == 0) return DD_OK;
  const int n_chunk = (F + 63) / 64;
  const dim3 grid((unsigned)(((long)n_seg * n_chunk + 3) / 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (op) {
    case dd::OP_SUM: hipLaunchKernelGGL(dd::k_segment_reduce<dd::OP_SUM>, grid, block, 0, st, src, seg_ptr, n_seg, F, n_chunk, out, arg_out, E); break;
    case dd::OP_MEAN: hipLaunchKernelGGL(dd::k_segment_reduce<dd::OP_MEAN>, grid, block, 0, st, src, seg_ptr, n_seg, F, n_chunk, out, arg_out, E); break;
    case dd::OP_MIN: hipLaunchKernelGGL(dd::k_segment_reduce<dd::OP_MIN>, grid, block, 0, st, src, seg_ptr, n_seg, F, n_chunk, out, arg_out, E); break;
    default: hipLaunchKernelGGL(dd::k_segment_reduce<dd::OP_MAX>, grid, block, 0, st, src, seg_ptr, n_seg, F, n_chunk, out, arg_out, E); break;
  }
  DD_CHECK_LAUNCH();
  return DD_OK;
}

extern "C" int dd_segment_softmax(const float* src, const int32_t* seg_ptr, int n_seg, int F, float* out, void* stream) {
  if (!seg_ptr || n_seg < 0 || F <= 0) return DD_ERR_BAD_ARG;
  if (n_seg == 0) return DD_OK;
  if (!src || !out) return DD_ERR_BAD_ARG;
  const int n_chunk = (F + 63) / 64;
  hipLaunchKernelGGL(dd::k_segment_softmax, dim3((unsigned)(((long)n_seg * n_chunk + 3) / 4)), dim3(256), 0, (hipStream_t)stream, src,
                     seg_ptr, n_seg, F, n_chunk, out);
  DD_CHECK_LAUNCH();
  return DD_OK;
}
