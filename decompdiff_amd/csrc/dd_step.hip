// Reverse-diffusion step kernels (models/decompdiff.py:601-689, models/transitions.py:65-161)
// and drift guidance with analytic gradients (utils/guidance_funcs.py:24-78).
//
//   step_row       one wave per ligand atom / per bond row: type head second Linear
//                  (ShiftedSoftplus -> Linear, decompdiff.py:194-211), log_softmax, categorical
//                  posterior q(v_{t-1}|v_t, v0) in log space, Gumbel-argmax sample, trajectories.
//   step_pos_elem  one thread per ligand coordinate: C0 posterior mean, drift, noise.
//   k_step_all     both in one launch per step (block ranges); k_step_rows / k_step_pos: each as a launch of its own
//                  (dd_reverse_step, where the host supplies the logits, and the measurement build).
//   forward_row    one wave per row: a class drawn from the forward process or the prior (k_jump, k_chain_init).
//   k_drift_*      gradients of the armsca_prox / clash / arms_repul energies at x_t, and of the caller's distance restraints
//                  (k_drift_restraint, EXTENSION: points in the pocket that an atom or the nearest atom of a group must keep to;
//                  its GENERAL instantiation adds typed atoms, ligand pairs, the harmonic form and per-step rows).
// The current step index lives in device memory (step_counter) so that one captured hipGraph
// can be replayed for every step.
#include <string.h>
#include <type_traits>
#include <vector>

#include "dd_kernels.hpp"

namespace dd {

// Production noise (Philox4x32-10, counter = (row, row >> 32, t, stream id)): one uniform per (row, class) for the
// Gumbel draws -- classes 4k..4k+3 from the block of stream `sid | (k << 8)` (8 classes: two blocks, up to 23 classes of
// ligand_atom_mode 'full': six) -- and one
// Box-Muller normal per coordinate (stream 7).  Streams: 1 atom types, 2 bond types, 7 coordinates; distinct
// (row, t, stream) never share a counter.  `t` is the diffusion time index of the step (t_start - steps done), not the
// step number of the call: a chain resumed with start_step and the same seed continues the noise of the unsplit chain
// (tests/test_gpu_properties.py) instead of replaying the draws of its first steps.  dd_debug_philox exposes exactly these functions to the statistics test.
// `seed` and `row` are the run state's seed and the flat row of the batch, or -- keyed chains -- the sample's key and the row of its
// own enumeration (noise_addr below): the same generator either way.
// Resampling (dd_resample): a chain that jumps back visits a time again, so the time word of a FIXED step is t + 65536 * epoch
// (epoch = jumps done so far in the call; epoch 0: the bits above), and the jump that raises the epoch to e draws at
// (l + j) + 65536 * e on streams of its own: 3 atom types, 4 bond types, 8 coordinates (same class blocks, same row addressing).
// Chain init (dd_init): the chain's first level is drawn at the time word of that level (T, or t_start of a noised init) on streams
// 5 atom types, 6 bond types, 9 coordinates.
template <int NC>
__device__ __forceinline__ float philox_uniform(uint64_t seed, long row, int step, uint32_t sid, int c) {
  Philox ph(seed);
  uint32_t bits = 0u;
#pragma unroll
  for (int blk = 0; blk < (NC + 3) / 4; ++blk) {
    uint32_t r[4];
    ph.gen((uint32_t)row, (uint32_t)(row >> 32), (uint32_t)step, sid | ((uint32_t)blk << 8), r);
#pragma unroll
    for (int k = 0; k < 4; ++k) bits = (c == 4 * blk + k) ? r[k] : bits;
  }
  return u01(bits);
}
__device__ __forceinline__ float philox_normal(uint64_t seed, int idx, int step, uint32_t sid = 7u) {
  Philox ph(seed);
  uint32_t r[4];
  ph.gen((uint32_t)idx, 0u, (uint32_t)step, sid, r);
  const float u1 = fmaxf(u01(r[0]), 5.9604645e-8f), u2 = u01(r[1]);
  return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}


// Run state in device memory (dd_sampler.step_counter, [4] int32: steps done, t_start, seed lo, seed hi; written by
// dd_sampler_reset): a captured step graph is replayed for every step AND re-used for the next chain of the same shape
// with another seed / start time -- nothing chain-specific is baked into its kernel arguments.
struct RunState { int step, t_start; uint64_t seed; };
__device__ __forceinline__ RunState load_run_state(const int32_t* __restrict__ rs, int counter_bias) {
  RunState r;
  r.step = rs[0] - counter_bias;
  r.t_start = rs[1];
  r.seed = (uint64_t)(uint32_t)rs[2] | ((uint64_t)(uint32_t)rs[3] << 32);
  return r;
}

// Where a row's draws come from.  Unkeyed (a.sample_keys == NULL): the run state's seed and the flat row of the batch.  Keyed
// (dd_sample_steps_keyed): sample b = row / rows_per_sample draws with its own key at the row of its OWN dense enumeration, i.e.
// what a batch of that sample alone with seed = key draws -- atoms: the index in the sample; bonds of a padded batch: the
// padded row dst * (NL - 1) + sp is row dst * (n - 1) + sp of the sample's n = nl_real[b] atoms (padding rows keep theirs).
struct NoiseAddr { uint64_t key; long row; };
__device__ __forceinline__ NoiseAddr noise_addr(const StepRowsArgs& a, const long row, const uint64_t seed) {
  if (a.sample_keys == nullptr) return {seed, row};
  const int b = (int)(row / a.rows_per_sample);
  int r = (int)(row - (long)b * a.rows_per_sample);
  if (a.nl_real != nullptr) {
    const int n = a.nl_real[b], dst = r / (a.NL - 1), sp = r - dst * (a.NL - 1);
    if (dst < n && sp < n - 1) r = dst * (n - 1) + sp;    // (sp < n - 1 and dst < n: both endpoints are real atoms)
  }
  return {a.sample_keys[b], (long)r};
}
// ... and a coordinate's: (seed, flat index), or (key of its sample, 3 * i + c inside the sample)
__device__ __forceinline__ float step_pos_normal(const StepPosArgs& a, const int idx, const int b, const uint64_t seed, const int t,
                                                 const uint32_t sid = 7u) {
  if (a.sample_keys == nullptr) return philox_normal(seed, idx, t, sid);
  return philox_normal(a.sample_keys[b], idx - b * a.NL * 3, t, sid);
}
// the Philox time word of a step at time t (or of a jump to level t) in the chain's current epoch
__device__ __forceinline__ int epoch_word(const int32_t* __restrict__ epoch, const int t) {
  return epoch == nullptr ? t : (int)((uint32_t)t + ((uint32_t)*epoch << 16));
}

__device__ __forceinline__ float log_add_exp(float a, float b) {
  float m = fmaxf(a, b);
  return m + logf(expf(a - m) + expf(b - m));
}

// ---- fixed atoms (include/decompdiff_hip.h, dd_fixed).  FIXED instantiations only; the others carry none of this.
// A held atom row: its mask byte; a held bond row: both endpoints' bytes (row r of a sample: dst = r / (NL - 1),
// sp = r % (NL - 1), src = sp + (sp >= dst)).  Padding atoms carry 0, so no bond that touches one is held.
__device__ __forceinline__ bool row_held(const StepRowsArgs& a, const long row) {
  if (!a.fx_bond) return a.fx_mask[row] != 0;
  const int b = (int)(row / a.rows_per_sample);
  const int r = (int)(row - (long)b * a.rows_per_sample);
  const int dst = r / (a.NL - 1), sp = r - dst * (a.NL - 1), src = sp + (sp >= dst ? 1 : 0);
  const uint8_t* m = a.fx_mask + (long)b * a.NL;
  return m[dst] != 0 && m[src] != 0;
}
// log q(v_l | v0) of the forward process for class c with the CLEAN one-hot (transitions.py:146-150): the q0 of the step with
// log(clamp(onehot, 1e-30)) in place of the prediction; lca / l1mca at level l
__device__ __forceinline__ float fixed_q0(const bool is_v0, const float lca, const float l1mca, const float log_prior) {
  return log_add_exp((is_v0 ? 0.f : -69.07755278982137f) + lca, l1mca + log_prior);
}
__device__ __forceinline__ float gumbel_of(const float u) { return -logf(-logf(u + 1e-30f) + 1e-30f); }
// the first class with the largest score of a row that holds one class per lane: class order, strict > (a serial loop's winner)
template <int NC>
__device__ __forceinline__ int class_argmax(const float sc) {
  int best = 0;
  float bestv = -INFINITY;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const float sk = lane_bcast(sc, k);
    if (sk > bestv) { bestv = sk; best = k; }
  }
  return best;
}
// x_l = A[l] (x0c - cc) + (S[l] e) std + cc (decompdiff.py:436-455 in the centred frame), every operation rounded on its own: the
// step, the initial level and every batch layout give the same bits
__device__ __forceinline__ float fixed_noised_pos(const float A, const float S, const float x0c, const float cc, const float e,
                                                  const float std) {
  return __fadd_rn(__fadd_rn(__fmul_rn(A, __fsub_rn(x0c, cc)), __fmul_rn(__fmul_rn(S, e), std)), cc);
}

__global__ void k_advance(int32_t* step_counter) { *step_counter += 1; }
__global__ void k_reset_run_state(int32_t* rs, int t_start, uint32_t seed_lo, uint32_t seed_hi) {
  rs[0] = 0; rs[1] = t_start; rs[2] = (int32_t)seed_lo; rs[3] = (int32_t)seed_hi;
}

// ------------------------------------------------------------------------------ drift: armsca
// Per sample: d_arm = min over (arm atom a in arm, scaffold atom s) |x_a - x_s|;
// loss = sum_b mean_arms( relu(min_d - d) + relu(d - max_d) ) / B       (guidance_funcs.py:50-78)
// One workgroup per sample: 64 threads (NL <= 64: one wave, the reduction stays in registers) or 128 (NL <= 128: the two
// waves' winners meet in LDS).
__global__ __launch_bounds__(DD_NL_MAX) void k_drift_armsca(const float* __restrict__ pos, const int32_t* __restrict__ decomp,
                                                     int B, int NL, float min_d, float max_d, float* __restrict__ grad,
                                                     int accumulate, int norm_B) {
  __shared__ float px[DD_NL_MAX], py[DD_NL_MAX], pz[DD_NL_MAX];
  __shared__ int arm[DD_NL_MAX];
  __shared__ float gx[DD_NL_MAX], gy[DD_NL_MAX], gz[DD_NL_MAX];
  const int b = blockIdx.x, l = threadIdx.x;
  int my_arm = -2;
  if (l < NL) {
    px[l] = pos[((long)b * NL + l) * 3]; py[l] = pos[((long)b * NL + l) * 3 + 1]; pz[l] = pos[((long)b * NL + l) * 3 + 2];
    my_arm = decomp[(long)b * NL + l];
    arm[l] = my_arm;
    gx[l] = 0.f; gy[l] = 0.f; gz[l] = 0.f;
  }
  __syncthreads();
  // number of arms = max id + 1 (scatter_min output rows); a sample is "valid" iff it has arm and scaffold atoms
  int n_arms = 0, n_sca = 0, n_armatoms = 0;
  for (int i = 0; i < NL; ++i) {
    n_arms = arm[i] + 1 > n_arms ? arm[i] + 1 : n_arms;
    n_sca += arm[i] == -1;
    n_armatoms += arm[i] >= 0;
  }
  if (n_sca > 0 && n_armatoms > 0) {
    // One arm at a time, one lane per scaffold atom (the serial form -- one lane per ARM walking all NL x NL pairs -- kept
    // two lanes busy for 54 us per step).  Same arithmetic and the same winners: lane s finds the nearest atom of the arm
    // (ascending i, strict <: the first minimum, as scatter_min), then the wave takes the (distance, s) lexicographic
    // minimum -- the first scaffold atom at the smallest distance, which is what the ascending strict-< loop over s picked.
    for (int a = 0; a < n_arms; ++a) {
      float bcol = INFINITY;
      int bca = -1;
      if (l < NL && my_arm == -1) {
        for (int i = 0; i < NL; ++i) {
          if (arm[i] != a) continue;
          float dx = px[i] - px[l], dy = py[i] - py[l], dz = pz[i] - pz[l];
          float d = sqrtf(dx * dx + dy * dy + dz * dz);
          if (d < bcol) { bcol = d; bca = i; }
        }
      }
      unsigned key = __float_as_uint(bcol);                // d >= 0 (or +inf): unsigned order = float order
      int who = l;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned k2 = (unsigned)__shfl_xor((int)key, off);
        const int w2 = __shfl_xor(who, off);
        if (k2 < key || (k2 == key && w2 < who)) { key = k2; who = w2; }
      }
      int ba = __shfl(bca, who & 63);                      // this wave's winner and its arm atom
      if (blockDim.x > 64) {                               // 65 .. 128 ligand atoms: second wave's winner through LDS
        __shared__ unsigned wk[2];
        __shared__ int ww[2], wa[2];
        __syncthreads();                                   // (previous arm's readers are done)
        if ((l & 63) == 0) { wk[l >> 6] = key; ww[l >> 6] = who; wa[l >> 6] = ba; }
        __syncthreads();
        const int pick = (wk[1] < wk[0] || (wk[1] == wk[0] && ww[1] < ww[0])) ? 1 : 0;
        key = wk[pick]; who = ww[pick]; ba = wa[pick];
      }
      const float best = __uint_as_float(key);
      const int bs = who;
      if (l == 0 && ba >= 0) {
        // The clamps pass their gradient at equality (torch.clamp backward is inclusive; min_d == max_d == d: the two
        // cancel), and a winner at distance 0 gives nothing (torch's norm has a zero subgradient there), as in arms_repul.
        float coef = 0.f;
        if (min_d - best >= 0.f) coef -= 1.f;
        if (best - max_d >= 0.f) coef += 1.f;
        coef /= ((float)n_arms * (float)norm_B);          // the loss is averaged over the caller's whole batch
        if (coef != 0.f && best > 0.f) {
          float dx = px[ba] - px[bs], dy = py[ba] - py[bs], dz = pz[ba] - pz[bs];
          float inv = 1.0f / best;
          // (products rounded before the add, as the atomic adds of the serial form took them; arms in ascending order,
          //  as its lane-ordered atomics)
          const float tx = __fmul_rn(__fmul_rn(coef, dx), inv), ty = __fmul_rn(__fmul_rn(coef, dy), inv), tz = __fmul_rn(__fmul_rn(coef, dz), inv);
          const float ux = __fmul_rn(__fmul_rn(-coef, dx), inv), uy = __fmul_rn(__fmul_rn(-coef, dy), inv), uz = __fmul_rn(__fmul_rn(-coef, dz), inv);
          gx[ba] = __fadd_rn(gx[ba], tx); gy[ba] = __fadd_rn(gy[ba], ty); gz[ba] = __fadd_rn(gz[ba], tz);
          gx[bs] = __fadd_rn(gx[bs], ux); gy[bs] = __fadd_rn(gy[bs], uy); gz[bs] = __fadd_rn(gz[bs], uz);
        }
      }
    }
  }
  __syncthreads();
  if (l < NL) {
    float* g = grad + ((long)b * NL + l) * 3;
    if (accumulate) { g[0] += gx[l]; g[1] += gy[l]; g[2] += gz[l]; }
    else { g[0] = gx[l]; g[1] = gy[l]; g[2] = gz[l]; }
  }
}

// ------------------------------------------------------------------------------ drift: arms_repul
// compute_batch_arms_repul_loss (guidance_funcs.py:81-118), analytic gradient.  Per sample, for every arm pair a1 <= a2 (the
// reference's loop INCLUDES a1 == a2) with atoms on both sides, d_pq = |x_p - x_q| over p in a1, q in a2:
//   mode 1 'min': relu(max_d - min_pq d_pq)          -> d/dx_p = -(x_p - x_q)/d at the arg-min pair (first minimum in (p, q)
//                 order; torch splits the gradient evenly over exact ties), nothing for a1 == a2 (the minimum is a zero on
//                 the diagonal and torch's norm has a zero subgradient there);
//   mode 2 'all': mean_pq relu(max_d - d_pq)         -> d/dx_p = -(x_p - x_q) / (d n1 n2) for every pair inside max_d; the
//                 pairs of one arm appear as (p, q) and (q, p): twice the weight, and the diagonal (d = 0) gives nothing.
// The sum over pairs and samples is divided by the batch size.  The clamp passes its gradient where max_d - d >= 0
// (torch.clamp backward is inclusive).  One workgroup per sample, one thread per ligand atom.
__global__ __launch_bounds__(DD_NL_MAX) void k_drift_arms_repul(const float* __restrict__ pos, const int32_t* __restrict__ decomp, int B,
                                                                int NL, float max_d, int mode, float* __restrict__ grad,
                                                                int accumulate, int norm_B) {
  __shared__ float px[DD_NL_MAX], py[DD_NL_MAX], pz[DD_NL_MAX];
  __shared__ int arm[DD_NL_MAX];
  __shared__ unsigned long long best[DD_NL_MAX];           // mode 1: per atom p of a1 the key (bits(d), q) of its nearest atom of a2
  __shared__ float gx[DD_NL_MAX], gy[DD_NL_MAX], gz[DD_NL_MAX];
  const int b = blockIdx.x, l = threadIdx.x;
  int my_arm = -2;
  if (l < NL) {
    px[l] = pos[((long)b * NL + l) * 3]; py[l] = pos[((long)b * NL + l) * 3 + 1]; pz[l] = pos[((long)b * NL + l) * 3 + 2];
    my_arm = decomp[(long)b * NL + l];
    arm[l] = my_arm;
    gx[l] = 0.f; gy[l] = 0.f; gz[l] = 0.f;
  }
  __syncthreads();
  int n_arms = 0;                                          // mask.max() + 1 (guidance_funcs.py:99)
  for (int i = 0; i < NL; ++i) n_arms = arm[i] + 1 > n_arms ? arm[i] + 1 : n_arms;
  const float inv_B = 1.0f / (float)norm_B;
  if (mode == 2) {
    // every atom gathers its own gradient: sum over the atoms q of every arm (its own included), ascending q
    if (l < NL && my_arm >= 0) {
      int n_mine = 0;
      for (int i = 0; i < NL; ++i) n_mine += arm[i] == my_arm;
      float ax = 0.f, ay = 0.f, az = 0.f;
      for (int a2 = 0; a2 < n_arms; ++a2) {
        int n2 = 0;
        for (int i = 0; i < NL; ++i) n2 += arm[i] == a2;
        if (n2 == 0) continue;
        const float w = (a2 == my_arm ? 2.0f : 1.0f) / ((float)n_mine * (float)n2) * inv_B;
        for (int q = 0; q < NL; ++q) {
          if (arm[q] != a2 || q == l) continue;
          const float dx = px[l] - px[q], dy = py[l] - py[q], dz = pz[l] - pz[q];
          const float d = sqrtf(dx * dx + dy * dy + dz * dz);
          if (max_d - d >= 0.f && d > 0.f) {
            const float c = -w / d;
            ax = fmaf(c, dx, ax); ay = fmaf(c, dy, ay); az = fmaf(c, dz, az);
          }
        }
      }
      gx[l] = ax; gy[l] = ay; gz[l] = az;
    }
  } else {
    for (int a1 = 0; a1 < n_arms; ++a1) {
      for (int a2 = a1 + 1; a2 < n_arms; ++a2) {           // (a1 == a2: zero gradient, see above)
        unsigned long long key = ~0ull;
        if (l < NL && my_arm == a1) {
          for (int q = 0; q < NL; ++q) {
            if (arm[q] != a2) continue;
            const float dx = px[l] - px[q], dy = py[l] - py[q], dz = pz[l] - pz[q];
            const float d = sqrtf(dx * dx + dy * dy + dz * dz);
            const unsigned long long k = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)q;   // d >= 0: bit order = float order
            key = k < key ? k : key;
          }
        }
        if (l < NL) best[l] = key;
        __syncthreads();
        if (l == 0) {
          unsigned long long bk = ~0ull;
          int bp = -1;
          for (int p = 0; p < NL; ++p)
            if (best[p] < bk) { bk = best[p]; bp = p; }     // strict <: the first p at the smallest distance
          if (bp >= 0 && (unsigned)(bk >> 32) != 0xffffffffu) {
            const float d = __uint_as_float((unsigned)(bk >> 32));
            const int q = (int)(unsigned)(bk & 0xffffffffull);
            if (max_d - d >= 0.f && d > 0.f) {
              const float c = -inv_B / d;
              const float dx = px[bp] - px[q], dy = py[bp] - py[q], dz = pz[bp] - pz[q];
              gx[bp] = fmaf(c, dx, gx[bp]); gy[bp] = fmaf(c, dy, gy[bp]); gz[bp] = fmaf(c, dz, gz[bp]);
              gx[q] = fmaf(-c, dx, gx[q]); gy[q] = fmaf(-c, dy, gy[q]); gz[q] = fmaf(-c, dz, gz[q]);
            }
          }
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();
  if (l < NL) {
    float* g = grad + ((long)b * NL + l) * 3;
    if (accumulate) { g[0] += gx[l]; g[1] += gy[l]; g[2] += gz[l]; }
    else { g[0] = gx[l]; g[1] = gy[l]; g[2] = gz[l]; }
  }
}

// ------------------------------------------------------------------------------ drift: clash
// G_i = -sigma * log(1e-3 + sum_j exp(-|p_j - y_i|^2 / sigma)), y_i = x_i + offset_b
// loss = sum_b mean_i relu(gamma - G_i)   (guidance_funcs.py:24-42)
// dloss/dx_i = -(1/NL) [G_i < gamma] * 2/(1e-3+S) * sum_j e_j (y_i - p_j)
// One workgroup (256 threads) per ligand atom.
__global__ __launch_bounds__(256) void k_drift_clash(const float* __restrict__ pos, const float* __restrict__ offset,
                                                     const float* __restrict__ prot, int B, int NL, int NF, float sigma,
                                                     float gamma, float* __restrict__ grad, int accumulate,
                                                     const int32_t* __restrict__ nl_real) {
  __shared__ float red[4][4];
  const int atom = blockIdx.x, b = atom / NL;
  const int nlb = nl_real ? nl_real[b] : NL;             // the loss is the mean over the sample's REAL ligand atoms
  if (atom % NL >= nlb) {                                // padding atom of a heterogeneous batch
    if (threadIdx.x < 3 && !accumulate) grad[(long)atom * 3 + threadIdx.x] = 0.f;
    return;
  }
  const float yx = pos[(long)atom * 3] + offset[b * 3], yy = pos[(long)atom * 3 + 1] + offset[b * 3 + 1],
              yz = pos[(long)atom * 3 + 2] + offset[b * 3 + 2];
  const float* pb = prot + (long)b * NF * 3;
  float S = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
  const float inv_sigma = 1.0f / sigma;
  for (int j = threadIdx.x; j < NF; j += 256) {
    float dx = yx - pb[3 * j], dy = yy - pb[3 * j + 1], dz = yz - pb[3 * j + 2];
    float e = expf(-(dx * dx + dy * dy + dz * dz) * inv_sigma);
    S += e; sx = fmaf(e, dx, sx); sy = fmaf(e, dy, sy); sz = fmaf(e, dz, sz);
  }
  S = wave_sum(S); sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { red[wave][0] = S; red[wave][1] = sx; red[wave][2] = sy; red[wave][3] = sz; }
  __syncthreads();
  if (threadIdx.x < 3) {
    float St = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    float v = red[0][1 + threadIdx.x] + red[1][1 + threadIdx.x] + red[2][1 + threadIdx.x] + red[3][1 + threadIdx.x];
    float G = -sigma * logf(1e-3f + St);
    float g = 0.f;
    if (gamma - G > 0.f) g = -(1.0f / (float)nlb) * 2.0f / (1e-3f + St) * v;
    float* dst = grad + (long)atom * 3 + threadIdx.x;
    *dst = accumulate ? *dst + g : g;
  }
}

// ------------------------------------------------------------------------------ drift: restraint
// E = sum_r w_r (relu(min_d_r - d_r) + relu(d_r - max_d_r)), d_r = |x_w - p_r|, w the explicit atom of restraint r or the FIRST
// nearest member of its group in row order (include/decompdiff_hip.h, dd_restraints); no division by B or R.  One workgroup per
// sample, lane = atom: 64 threads (NL <= 64: the reduction stays in registers) or 128 (the two waves' winners meet in LDS, one
// 8-byte word each: key << 32 | row, double-buffered by the parity of the restraint so that one barrier per restraint is enough).
// The winning lane adds into its own registers, restraints in ascending order: no atomics, the same bits on every run.  The
// clamps pass their gradient at equality, a winner at distance 0 gives nothing (as k_drift_armsca), an empty group has distance
// +inf and winner -1.  Memory-safe for any contents of the restraint arrays: ptr is clamped to [0, R], an atom outside the
// sample matches no lane.  Outside the time window the gradient rows are zeros; dist / winner are reported either way.
//
// GENERAL (include/decompdiff_hip.h, "the general form"; the caller's struct carries a trailing array): on top of that class masks
// over the CURRENT atom classes, pair restraints between two ligand atoms, the harmonic hinge and one trajectory row per step; a
// linear untyped point restraint keeps the arithmetic above operation for operation.  The sample's coordinates, class bits and arm
// ids are staged in LDS once (128 x 5 words); a pair restraint has lane i (a member of set 1) scan the members j != i of set 2 in
// ascending order under strict <, then the workgroup reduces dist_bits << 32 | i << 8 | j, whose minimum is the first nearest pair
// in (i, j) order.  Both winning lanes add the SAME rounded products into their own registers (+ on i, - on j).  Memory-safe for
// any array contents: an atom outside the sample matches no j either, a class id outside [0, 32) has no bit.  The point
// instantiation carries none of this: no staging, no class, pair, form or trajectory code.
__device__ __forceinline__ bool restraint_member(int row, int n, int at, int gp, int arm, bool has_decomp, bool typed, unsigned cbit,
                                                 unsigned mask) {
  return row < n && (at >= 0 ? row == at : (gp == DD_RESTRAINT_ANY || (has_decomp && gp >= -1 && arm == gp))) &&
         (!typed || (cbit & mask) != 0u);
}
template <bool GENERAL>
__global__ __launch_bounds__(DD_NL_MAX) void k_drift_restraint(const RestraintArgs g) {
  // One struct under two names: `g.` reads the general form's fields, `a.` the point form's.  Reading both through one name
  // is the same program, but the compiler then orders the GENERAL instantiation's scalar code differently (8 instructions more).
  const RestraintArgs& a = g;
  __shared__ unsigned long long wk[2][2];
  __shared__ float sx[DD_NL_MAX], sy[DD_NL_MAX], sz[DD_NL_MAX];              // (these five: GENERAL only)
  __shared__ unsigned sbit[DD_NL_MAX];
  __shared__ int sarm[DD_NL_MAX];
  const int b = blockIdx.x, l = threadIdx.x, NL = a.NL;
  int n = a.nl_real ? a.nl_real[b] : NL;
  n = n < NL ? n : NL;
  float x = 0.f, y = 0.f, z = 0.f;
  int my_arm = -2;
  unsigned my_bit = 0u;
  if (l < n) {
    const float* p = a.pos + ((long)b * NL + l) * 3;
    x = p[0]; y = p[1]; z = p[2];
    if (a.decomp) my_arm = a.decomp[(long)b * NL + l];
    if constexpr (GENERAL) {
      if (g.lig_v) {
        const int c = g.lig_v[(long)b * NL + l];
        my_bit = c >= 0 && c < 32 ? 1u << c : 0u;
      }
    }
  }
  if constexpr (GENERAL) {
    sx[l] = x; sy[l] = y; sz[l] = z; sbit[l] = my_bit; sarm[l] = my_arm;     // (blockDim.x <= DD_NL_MAX)
    __syncthreads();
  }
  bool active = true;
  int trow = -1;
  if (a.step_counter != nullptr) {
    const RunState rs = load_run_state(a.step_counter, a.counter_bias);
    const int t = rs.t_start - rs.step;
    active = t >= a.t_min && t <= a.t_max;
    if constexpr (GENERAL) {
      if (rs.step >= 0 && rs.step < g.traj_positions) trow = rs.step;
    }
  }
  const bool traj = GENERAL ? trow >= 0 && (g.dist_traj != nullptr || g.winner_traj != nullptr || g.winner2_traj != nullptr) : false;
  int r0 = a.ptr[b], r1 = a.ptr[b + 1];
  r0 = r0 < 0 ? 0 : (r0 > a.R ? a.R : r0);
  r1 = r1 < r0 ? r0 : (r1 > a.R ? a.R : r1);
  if constexpr (GENERAL) {                                 // (inactive and nothing to report: no restraint is visited)
    if (!active && !traj && a.dist == nullptr && a.winner == nullptr && g.winner2 == nullptr) r1 = r0;
  } else {
    if (!active && a.dist == nullptr && a.winner == nullptr) r1 = r0;
  }
  const bool has_decomp = a.decomp != nullptr;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  for (int r = r0; r < r1; ++r) {                          // (r0, r1: the same in every thread of the workgroup)
    const int at = a.atom[r], gp = a.group[r];
    const bool mine = GENERAL ? restraint_member(l, n, at, gp, my_arm, has_decomp, g.cls != nullptr, my_bit, g.cls ? g.cls[r] : 0u)
                              : l < n && (at >= 0 ? l == at : (gp == DD_RESTRAINT_ANY || (a.decomp != nullptr && gp >= -1 && my_arm == gp)));
    const bool is_pair = GENERAL ? g.pair != nullptr && g.pair[r] != 0 : false;
    float dx, dy, dz, d = INFINITY;
    unsigned long long key;
    if (!is_pair) {
      dx = x - a.point[3 * (long)r]; dy = y - a.point[3 * (long)r + 1]; dz = z - a.point[3 * (long)r + 2];
      d = mine ? sqrtf(dx * dx + dy * dy + dz * dz) : INFINITY;
      key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)l;   // d >= 0 (or +inf): bit order = float order
    } else if constexpr (GENERAL) {
      const int at2 = g.atom2 ? g.atom2[r] : -1, gp2 = g.group2 ? g.group2[r] : DD_RESTRAINT_NONE;
      const bool typed2 = g.cls2 != nullptr;
      const unsigned m2 = typed2 ? g.cls2[r] : 0u;
      int j0 = 0, j1 = n, bj = 0;
      if (at2 >= 0) { j0 = at2 < n ? at2 : n; j1 = at2 < n ? at2 + 1 : n; }   // (an explicit second atom: one candidate)
      if (mine) {
        for (int j = j0; j < j1; ++j) {
          if (j == l || !restraint_member(j, n, at2, gp2, sarm[j], has_decomp, typed2, sbit[j], m2)) continue;
          const float ex = x - sx[j], ey = y - sy[j], ez = z - sz[j];
          const float dj = sqrtf(ex * ex + ey * ey + ez * ez);
          if (dj < d) { d = dj; bj = j; }
        }
      }
      key = ((unsigned long long)__float_as_uint(d) << 32) | ((unsigned)l << 8) | (unsigned)bj;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long k2 = (unsigned long long)__shfl_xor((long long)key, off);
      key = k2 < key ? k2 : key;
    }
    if (blockDim.x > 64) {
      if ((l & 63) == 0) wk[r & 1][l >> 6] = key;
      __syncthreads();
      const unsigned long long k0 = wk[r & 1][0], k1 = wk[r & 1][1];
      key = k1 < k0 ? k1 : k0;
    }
    const float best = __uint_as_float((unsigned)(key >> 32));
    const bool found = best < INFINITY || best != best;
    const unsigned low = (unsigned)(key & 0xffffffffull);
    const int win = found ? (int)(is_pair ? low >> 8 : low) : -1;
    const int win2 = found && is_pair ? (int)(low & 0xffu) : -1;
    if (l == 0) {
      if (a.dist) a.dist[r] = best;
      if (a.winner) a.winner[r] = win;
      if constexpr (GENERAL) {
        if (g.winner2) g.winner2[r] = win2;
        if (traj) {
          const long o = (long)trow * a.R + r;
          if (g.dist_traj) g.dist_traj[o] = best;
          if (g.winner_traj) g.winner_traj[o] = win;
          if (g.winner2_traj) g.winner2_traj[o] = win2;
        }
      }
    }
    if (active && (GENERAL ? found && (l == win || l == win2) : l == win)) {
      float coef = 0.f;
      if constexpr (GENERAL) {
        const float w = a.weight[r];
        if (g.form != nullptr && g.form[r] != 0) {
          const float lo = a.min_d[r] - best, hi = best - a.max_d[r];
          if (lo > 0.f) coef -= 2.f * w * lo;
          if (hi > 0.f) coef += 2.f * w * hi;
        } else {
          if (a.min_d[r] - best >= 0.f) coef -= 1.f;
          if (best - a.max_d[r] >= 0.f) coef += 1.f;
          coef *= w;
        }
      } else {
        if (a.min_d[r] - best >= 0.f) coef -= 1.f;
        if (best - a.max_d[r] >= 0.f) coef += 1.f;
        coef *= a.weight[r];
      }
      if (coef != 0.f && best > 0.f) {
        const float inv = 1.0f / best;
        if constexpr (GENERAL) {
          if (is_pair) {                                     // (both ends form the same three products from LDS: exactly opposite)
            dx = sx[win] - sx[win2]; dy = sy[win] - sy[win2]; dz = sz[win] - sz[win2];
          }
        }
        const float tx = __fmul_rn(__fmul_rn(coef, dx), inv), ty = __fmul_rn(__fmul_rn(coef, dy), inv), tz = __fmul_rn(__fmul_rn(coef, dz), inv);
        if (l == win) { gx = __fadd_rn(gx, tx); gy = __fadd_rn(gy, ty); gz = __fadd_rn(gz, tz); }
        else { gx = __fadd_rn(gx, -tx); gy = __fadd_rn(gy, -ty); gz = __fadd_rn(gz, -tz); }
      }
    }
  }
  if (l < NL) {
    float* g = a.grad + ((long)b * NL + l) * 3;
    if (a.accumulate) { g[0] += gx; g[1] += gy; g[2] += gz; }
    else { g[0] = gx; g[1] = gy; g[2] = gz; }
  }
}
int launch_drift_restraint(const RestraintArgs& a, hipStream_t st) {
  if (a.B <= 0 || a.NL <= 0 || a.NL > DD_NL_MAX || a.R < 0) return DD_ERR_BAD_ARG;
  const dim3 grid(a.B), block(a.NL > 64 ? 128 : 64);
  if (a.general) hipLaunchKernelGGL(k_drift_restraint<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(k_drift_restraint<false>, grid, block, 0, st, a);
  DD_CHECK_LAUNCH();
  return DD_OK;
}

// ---------------------------------------------------------------------------------- one launch per reverse step
// Bond rows, atom rows and the coordinate update are independent given the head activations, so they share one
// launch (block ranges); the step counter is advanced by a 1-thread launch behind it (a last-block ticket was
// tried: ~1800 atomics on one address serialise to 45 us).  A row is one wave: the
// second head Linear uses the whole wave, the per-class posterior / Gumbel arithmetic runs one class per lane with
// the cross-class sums taken in class order through v_readlane (the sums of a serial loop over the classes, bit for bit).
// LOGITS_IN (dd_reverse_step): the host supplies the head outputs in a.logits_in; hid / W2 / b2 are not read.
template <int NC, bool FIXED, bool LOGITS_IN = false>
__device__ __forceinline__ void step_row(const StepRowsArgs& a, const long row, const int lane, const RunState rs) {
  const int step = rs.step, t = rs.t_start - step;
  float logit[NC];
  if constexpr (LOGITS_IN) {
#pragma unroll
    for (int c = 0; c < NC; ++c) logit[c] = a.logits_in[row * NC + c];
  } else {
    // ShiftedSoftplus (common.py:66-72): softplus(x) - log 2, torch threshold 20
    float2 hv = *reinterpret_cast<const float2*>(a.hid + row * 128 + 2 * lane);
    hv.x = (hv.x > 20.f ? hv.x : log1pf(expf(hv.x))) - 0.6931471805599453f;
    hv.y = (hv.y > 20.f ? hv.y : log1pf(expf(hv.y))) - 0.6931471805599453f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float2 w = *reinterpret_cast<const float2*>(a.W2 + c * 128 + 2 * lane);
      logit[c] = wave_sum(fmaf(hv.y, w.y, hv.x * w.x)) + a.b2[c];
    }
  }
  const int c = lane < NC ? lane : NC - 1;               // lanes >= NC shadow the last class (results unused)
  float mine = logit[0], mx = logit[0];
#pragma unroll
  for (int k = 1; k < NC; ++k) { mine = (c == k) ? logit[k] : mine; mx = fmaxf(mx, logit[k]); }
  const float e = expf(mine - mx);
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < NC; ++k) se += lane_bcast(e, k);
  // (x - max) - log(sum), as torch's log_softmax: x - (max + log(sum)) rounds the sum at the size of the logits, which costs the
  //  leading class half an ulp of max (1.2e-4 at logits of a few thousand) and carries into the posterior
  const float lsum = logf(se);
  const int tm1 = t - 1 < 0 ? 0 : t - 1;
  const float la_t = a.tab[t], l1ma_t = a.tab[a.T + t];
  const float lca = a.tab[2 * a.T + tm1], l1mca = a.tab[3 * a.T + tm1];
  const float log_prior = a.tab[4 * a.T + c];            // log prior of this lane's class (uniform: -log NC)
  const int cur = a.state[row];
  const float lv0 = (mine - mx) - lsum;
  const float lvt = (c == cur) ? 0.f : -69.07755278982137f;      // log(clamp(onehot, 1e-30))
  const float q0 = log_add_exp(lv0 + lca, l1mca + log_prior);    // q(v_{t-1} | v0)
  const float q1 = log_add_exp(lvt + la_t, l1ma_t + log_prior);  // q(v_t | v_{t-1})
  const float un = q0 + q1;
  float umax = -INFINITY;
#pragma unroll
  for (int k = 0; k < NC; ++k) umax = fmaxf(umax, lane_bcast(un, k));
  const float ue = expf(un - umax);
  float us = 0.f;
#pragma unroll
  for (int k = 0; k < NC; ++k) us += lane_bcast(ue, k);
  const float ulse = umax + logf(us);
  float u;
  if (a.uniforms) {
    u = a.uniforms[((long)step * a.rows + row) * NC + c];
  } else {
    const NoiseAddr na = noise_addr(a, row, rs.seed);
    int tw = t;
    if constexpr (FIXED) tw = epoch_word(a.epoch, t);
    u = philox_uniform<NC>(na.key, na.row, tw, a.stream_id, c);
  }
  const float lp = un - ulse;
  float sc = gumbel_of(u) + lp;                                  // Gumbel-argmax (transitions.py:78-84)
  int v0 = -1;                                                   // FIXED, held row (wave-uniform): its known class
  if constexpr (FIXED) {
    if (row_held(a, row)) {
      v0 = a.fx_val[row];
      // replace: the row's draw of this step decides the forward sample of the clean class at level t - 1 instead
      if (a.fx_mode == DD_FIXED_REPLACE && t > 0) sc = gumbel_of(u) + fixed_q0(c == v0, lca, l1mca, log_prior);
    }
  }
  int best = 0;                                                  // (class_argmax, written out: the call schedules k_step_all anew)
  float bestv = -INFINITY;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const float sk = lane_bcast(sc, k);
    if (sk > bestv) { bestv = sk; best = k; }
  }
  if constexpr (FIXED) {
    if (v0 >= 0 && (a.fx_mode != DD_FIXED_REPLACE || t == 0)) best = v0;
  }
  if (lane < NC) {
    if (a.logits_out) a.logits_out[row * NC + c] = mine;
    if (a.traj_recon) a.traj_recon[((long)step * a.rows + row) * NC + c] = lv0;
    if (a.traj_prob) a.traj_prob[((long)step * a.rows + row) * NC + c] = lp;
  }
  if (lane == 0) {
    a.state[row] = best;
    if (a.traj_state) a.traj_state[(long)step * a.rows + row] = best;
  }
}

template <bool FIXED>
__device__ __forceinline__ void step_pos_elem(const StepPosArgs& a, const int idx, const RunState rs) {
  const int n = a.B * a.NL * 3;
  if (idx >= n) return;
  const int step = rs.step, t = rs.t_start - step;
  const int atom = idx / 3, c = idx % 3, b = atom / a.NL;
  const float xt = a.xt[idx];
  float x0;
  if (a.x0_prev != nullptr) {
    const int r = idx % (a.NL * 3);
    x0 = a.x0_prev[((long)b * (a.NP + a.NL) + a.NP) * 3 + r] + a.x0_dxe[idx] + a.x0_dxb[idx];
    a.x0_out[idx] = x0;
  } else {
    x0 = a.x0[idx];
  }
  float mean = a.tab_pos[t] * x0 + a.tab_pos[a.T + t] * xt;
  float g = 0.f;
  if (a.grad_a) g += a.scale_a ? a.grad_a[idx] * a.tab_score[t] : a.grad_a[idx];
  if (a.grad_c) g += a.scale_c ? a.grad_c[idx] * a.tab_score[t] : a.grad_c[idx];
  if (a.grad_r) g += a.scale_r ? a.grad_r[idx] * a.tab_score[t] : a.grad_r[idx];
  if (a.grad_q) g += a.scale_q ? a.grad_q[idx] * a.tab_score[t] : a.grad_q[idx];
  mean -= g;
  float e;
  if (a.eps) {
    e = a.eps[(long)step * n + idx];
  } else {
    int tw = t;
    if constexpr (FIXED) tw = epoch_word(a.epoch, t);
    e = step_pos_normal(a, idx, b, rs.seed, tw);
  }
  const float nz = t == 0 ? 0.f : 1.f;
  float nxt = mean + nz * expf(0.5f * a.tab_pos[2 * a.T + t]) * e * a.atom_std[idx];
  if constexpr (FIXED) {
    if (a.fx_mask[atom] != 0) {
      nxt = a.fx_x0c[idx];                                 // hold, and the replace step at t = 0
      if (a.fx_mode == DD_FIXED_REPLACE && t > 0)
        nxt = fixed_noised_pos(a.fx_tab[t - 1], a.fx_tab[a.T + t - 1], nxt, a.fx_cc[idx], e, a.atom_std[idx]);
    }
  }
  a.xt[idx] = nxt;
  if (a.traj_pos) a.traj_pos[(long)step * n + idx] = nxt + a.offset[b * 3 + c];
}

template <int NV, bool FIXED>
__global__ __launch_bounds__(256) void k_step_all(const StepRowsArgs rb, const StepRowsArgs rv, const StepPosArgs p, int nb_b, int nb_v) {
  const int blk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const RunState rs = load_run_state(rb.step_counter, rb.counter_bias);
  if (blk < nb_b) {
    const long row = (long)blk * 4 + wave;
    if (row < rb.rows) step_row<DD_NUM_B, FIXED>(rb, row, lane, rs);
  } else if (blk < nb_b + nb_v) {
    const long row = (long)(blk - nb_b) * 4 + wave;
    if (row < rv.rows) step_row<NV, FIXED>(rv, row, lane, rs);
  } else {
    step_pos_elem<FIXED>(p, (blk - nb_b - nb_v) * 256 + threadIdx.x, rs);
  }
}

// The same two as launches of their own: dd_reverse_step, whose logits come from the host (unfixed chains only), and the
// measurement build's unfused step.
template <int NC, bool FIXED>
__global__ __launch_bounds__(256) void k_step_rows(const StepRowsArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const RunState rs = load_run_state(a.step_counter, a.counter_bias);
  if constexpr (!FIXED) {
    if (a.logits_in != nullptr) { step_row<NC, false, true>(a, row, lane, rs); return; }
  }
  step_row<NC, FIXED>(a, row, lane, rs);
}
template <bool FIXED>
__global__ void k_step_pos(const StepPosArgs a) {
  step_pos_elem<FIXED>(a, blockIdx.x * blockDim.x + threadIdx.x, load_run_state(a.step_counter, a.counter_bias));
}

// The instantiation for a runtime class count and for fixed atoms (instantiations of their own: the others carry none of it).
// Atom classes: 8 (ligand_atom_mode 'basic'), 13 ('add_aromatic'), 23 ('full') -- utils/transforms.py:15-64,138-151.
// launch(nc, fixed) takes both as compile-time constants and returns a status.
template <int NC, class F>
static int with_fixed(const bool fixed, F&& launch) {
  return fixed ? launch(std::integral_constant<int, NC>(), std::true_type()) : launch(std::integral_constant<int, NC>(), std::false_type());
}
template <class F>
static int for_atom_classes(const int nc, const bool fixed, F&& launch) {
  if (nc == 8) return with_fixed<8>(fixed, launch);
  if (nc == 13) return with_fixed<13>(fixed, launch);
  if (nc == 23) return with_fixed<23>(fixed, launch);
  return DD_ERR_UNSUPPORTED_SHAPE;
}

int launch_step_all(const StepRowsArgs& rb, const StepRowsArgs& rv, const StepPosArgs& p, hipStream_t st) {
  if (rb.NC != DD_NUM_B) return DD_ERR_UNSUPPORTED_SHAPE;
  const int nb_b = (rb.rows + 3) / 4, nb_v = (rv.rows + 3) / 4, nb_p = (p.B * p.NL * 3 + 255) / 256;
  const dim3 grid(nb_b + nb_v + nb_p);
  return for_atom_classes(rv.NC, p.fx_mask != nullptr, [&](auto nv, auto fixed) -> int {
    hipLaunchKernelGGL((k_step_all<nv(), fixed()>), grid, dim3(256), 0, st, rb, rv, p, nb_b, nb_v);
    DD_CHECK_LAUNCH();
    return DD_OK;
  });
}

// Fixed atoms, in front of the first step (dd_fixed_init): one thread per bond row, atom row and coordinate.  Hold: the known
// values.  Replace: level l = t_start of the forward process with the formulas and streams of a step, drawn at Philox time
// l + 1 -- what the step at time l + 1 would have left.  Free rows are not touched.
template <int NC>
__device__ __forceinline__ void fixed_init_row(const StepRowsArgs& a, const long row, const RunState rs) {
  if (!row_held(a, row)) return;
  const int v0 = a.fx_val[row];
  int best = v0;
  if (a.fx_mode == DD_FIXED_REPLACE) {
    const int l = rs.t_start;
    const float lca = a.tab[2 * a.T + l], l1mca = a.tab[3 * a.T + l];
    const NoiseAddr na = noise_addr(a, row, rs.seed);
    float bestv = -INFINITY;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float u = philox_uniform<NC>(na.key, na.row, l + 1, a.stream_id, c);
      const float s = gumbel_of(u) + fixed_q0(c == v0, lca, l1mca, a.tab[4 * a.T + c]);
      if (s > bestv) { bestv = s; best = c; }
    }
  }
  a.state[row] = best;
}
template <int NV>
__global__ __launch_bounds__(256) void k_fixed_init(const StepRowsArgs rb, const StepRowsArgs rv, const StepPosArgs p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const RunState rs = load_run_state(rb.step_counter, 0);
  const long n = (long)p.B * p.NL * 3;
  if (i < rb.rows) {
    fixed_init_row<DD_NUM_B>(rb, i, rs);
  } else if (i < (long)rb.rows + rv.rows) {
    fixed_init_row<NV>(rv, i - rb.rows, rs);
  } else if (i < (long)rb.rows + rv.rows + n) {
    const int idx = (int)(i - rb.rows - rv.rows), atom = idx / 3;
    if (p.fx_mask[atom] == 0) return;
    float x = p.fx_x0c[idx];
    if (p.fx_mode == DD_FIXED_REPLACE) {
      const int l = rs.t_start;
      const float e = step_pos_normal(p, idx, atom / p.NL, rs.seed, l + 1);
      x = fixed_noised_pos(p.fx_tab[l], p.fx_tab[p.T + l], x, p.fx_cc[idx], e, p.atom_std[idx]);
    }
    p.xt[idx] = x;
  }
}
int launch_fixed_init(const StepRowsArgs& rb, const StepRowsArgs& rv, const StepPosArgs& p, hipStream_t st) {
  if (rb.NC != DD_NUM_B || p.fx_mask == nullptr) return DD_ERR_UNSUPPORTED_SHAPE;
  const long total = (long)rb.rows + rv.rows + (long)p.B * p.NL * 3;
  const dim3 grid((unsigned)((total + 255) / 256));
  return for_atom_classes(rv.NC, false, [&](auto nv, auto) -> int {
    hipLaunchKernelGGL(k_fixed_init<nv()>, grid, dim3(256), 0, st, rb, rv, p);
    DD_CHECK_LAUNCH();
    return DD_OK;
  });
}

// Resampling (include/decompdiff_hip.h, dd_resample): the forward jump q(x_m | x_l) from the chain's current level
// l = t_start - steps done (the run state's; -1 is the clean level) to m = l + j, for the coordinates, atom rows and bond rows of
// the batch in one launch.  jtab [6][T] at m: A, S (coordinates), lr / l1mr of the atom and of the bond schedule.  A row is one
// wave with one class per lane, as in step_row (bond rows dominate: B NL (NL - 1) rows of 5 classes); the cross-class argmax runs
// in class order through v_readlane with the strict > of the serial loops.  Hold mode leaves the held rows alone; replace mode
// moves every row (a held row at level m is then a valid forward sample of its clean value).  Draws: time word m + 65536 * e with
// e = the epoch AFTER this jump, streams 3 / 4 / 8, rows and keys addressed as the step addresses them.
// One class row drawn from the forward process (a jump, the chain init), one class per lane: the draw of (key, row, word, sid),
// gumbel(u) + log q(v | v0 = from) with lca / l1mca of the level (fixed_q0), or -- from_v0 false -- + the bare log prior; then the
// first argmax in class order, as the step's.
template <int NC>
__device__ __forceinline__ void forward_row(const StepRowsArgs& a, const long row, const int lane, const uint64_t seed, const int word,
                                            const uint32_t sid, const float* __restrict__ log_prior, const bool from_v0, const int from,
                                            const float lca, const float l1mca) {
  const int c = lane < NC ? lane : NC - 1;                         // lanes >= NC shadow the last class (results unused)
  const NoiseAddr na = noise_addr(a, row, seed);
  const float u = philox_uniform<NC>(na.key, na.row, word, sid, c);
  const float lp = log_prior[c];
  const float sc = gumbel_of(u) + (from_v0 ? fixed_q0(c == from, lca, l1mca, lp) : lp);
  const int best = class_argmax<NC>(sc);
  if (lane == 0) a.state[row] = best;
}
template <int NV>
__global__ __launch_bounds__(256) void k_jump(const StepRowsArgs rb, const StepRowsArgs rv, const StepPosArgs p,
                                              const float* __restrict__ jtab, const int j, int nb_b, int nb_v) {
  const int blk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const RunState rs = load_run_state(rb.step_counter, 0);
  const int T = p.T;
  const int m = rs.t_start - rs.step + j;                          // l + j
  if (m < 0 || m >= T) return;                                     // (the host checks the schedule; never index past the table)
  const int word = (int)((uint32_t)m + ((uint32_t)(*rb.epoch + 1) << 16));
  if (blk < nb_b) {
    const long row = (long)blk * 4 + wave;
    if (row >= rb.rows || (rb.fx_mode == DD_FIXED_HOLD && row_held(rb, row))) return;      // (wave-uniform)
    forward_row<DD_NUM_B>(rb, row, lane, rs.seed, word, 4u, rb.tab + 4 * T, true, rb.state[row], jtab[4 * T + m], jtab[5 * T + m]);
  } else if (blk < nb_b + nb_v) {
    const long row = (long)(blk - nb_b) * 4 + wave;
    if (row >= rv.rows || (rv.fx_mode == DD_FIXED_HOLD && row_held(rv, row))) return;
    forward_row<NV>(rv, row, lane, rs.seed, word, 3u, rv.tab + 4 * T, true, rv.state[row], jtab[2 * T + m], jtab[3 * T + m]);
  } else {
    const int idx = (blk - nb_b - nb_v) * 256 + threadIdx.x;
    if (idx >= p.B * p.NL * 3) return;
    const int atom = idx / 3;
    if (p.fx_mode == DD_FIXED_HOLD && p.fx_mask[atom] != 0) return;
    const float e = step_pos_normal(p, idx, atom / p.NL, rs.seed, word, 8u);
    p.xt[idx] = fixed_noised_pos(jtab[m], jtab[T + m], p.xt[idx], p.fx_cc[idx], e, p.atom_std[idx]);
  }
}
__global__ void k_jump_tail(int32_t* rs, int32_t* epoch, int j) { rs[1] += j; *epoch += 1; }
__global__ void k_reset_epoch(int32_t* epoch) { *epoch = 0; }

int launch_jump(const StepRowsArgs& rb, const StepRowsArgs& rv, const StepPosArgs& p, const float* jtab, int j, int32_t* epoch,
                hipStream_t st) {
  if (rb.NC != DD_NUM_B) return DD_ERR_UNSUPPORTED_SHAPE;
  return for_atom_classes(rv.NC, false, [&](auto nv, auto) -> int {
    if (p.fx_mask == nullptr || p.fx_cc == nullptr || jtab == nullptr || epoch == nullptr || rb.epoch != epoch || j < 1) return DD_ERR_BAD_ARG;
    const int nb_b = (rb.rows + 3) / 4, nb_v = (rv.rows + 3) / 4, nb_p = (p.B * p.NL * 3 + 255) / 256;
    hipLaunchKernelGGL(k_jump<nv()>, dim3(nb_b + nb_v + nb_p), dim3(256), 0, st, rb, rv, p, jtab, j, nb_b, nb_v);
    DD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_jump_tail, dim3(1), dim3(1), 0, st, const_cast<int32_t*>(rb.step_counter), epoch, j);
    DD_CHECK_LAUNCH();
    return DD_OK;
  });
}
int launch_reset_epoch(int32_t* epoch, hipStream_t st) {
  hipLaunchKernelGGL(k_reset_epoch, dim3(1), dim3(1), 0, st, epoch);
  DD_CHECK_LAUNCH();
  return DD_OK;
}

// Chain init (include/decompdiff_hip.h, dd_init): the chain's level in front of its first step, drawn for every REAL row of the
// batch in one launch laid out as k_jump (block ranges over bond rows, atom rows, coordinates; a type row is one wave with one
// class per lane).  PRIOR: x = cc + (e std), class = argmax gumbel(u_c) + log prior_c, drawn at Philox time T (the level above the
// first step).  NOISED: level l = t_start (the run state's) of the forward process of a known ligand, with the formulas of the
// held rows of replace mode (fixed_noised_pos / fixed_q0), drawn at Philox time l.  Streams of their own: 5 atom types, 6 bond
// types, 9 coordinates -- no counter is shared with a step (1 / 2 / 7), a jump (3 / 4 / 8) or k_fixed_init (a step's streams).
// Rows and keys are addressed as a step addresses them (noise_addr / step_pos_normal); padding rows of a padded batch -- the
// rows noise_addr leaves at their padded address -- keep what the host put there.
__device__ __forceinline__ bool bond_row_real(const StepRowsArgs& a, const long row) {
  if (a.nl_real == nullptr) return true;
  const int b = (int)(row / a.rows_per_sample);
  const int r = (int)(row - (long)b * a.rows_per_sample);
  const int n = a.nl_real[b], dst = r / (a.NL - 1), sp = r - dst * (a.NL - 1);
  return dst < n && sp < n - 1;
}
template <int NV>
__global__ __launch_bounds__(256) void k_chain_init(const StepRowsArgs rb, const StepRowsArgs rv, const StepPosArgs p, const ChainInitArgs ci,
                                                    int nb_b, int nb_v) {
  const int blk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const RunState rs = load_run_state(rb.step_counter, 0);
  const int T = p.T;
  const bool noised = ci.mode == DD_INIT_NOISED;
  const int l = noised ? rs.t_start : T;                           // the level drawn = the Philox time word
  if (noised && (l < 0 || l >= T)) return;                         // (the host checks the level; never index past the tables)
  if (blk < nb_b) {
    const long row = (long)blk * 4 + wave;
    if (row >= rb.rows || !bond_row_real(rb, row)) return;         // (wave-uniform)
    forward_row<DD_NUM_B>(rb, row, lane, rs.seed, l, 6u, ci.lp_b != nullptr ? ci.lp_b : rb.tab + 4 * T, noised, noised ? ci.b0[row] : 0,
                          noised ? rb.tab[2 * T + l] : 0.f, noised ? rb.tab[3 * T + l] : 0.f);
  } else if (blk < nb_b + nb_v) {
    const long row = (long)(blk - nb_b) * 4 + wave;
    if (row >= rv.rows) return;
    if (ci.nl_real != nullptr && (int)(row % p.NL) >= ci.nl_real[row / p.NL]) return;
    forward_row<NV>(rv, row, lane, rs.seed, l, 5u, ci.lp_v != nullptr ? ci.lp_v : rv.tab + 4 * T, noised, noised ? ci.v0[row] : 0,
                    noised ? rv.tab[2 * T + l] : 0.f, noised ? rv.tab[3 * T + l] : 0.f);
  } else {
    const int idx = (blk - nb_b - nb_v) * 256 + threadIdx.x;
    if (idx >= p.B * p.NL * 3) return;
    const int atom = idx / 3, b = atom / p.NL;
    if (ci.nl_real != nullptr && atom - b * p.NL >= ci.nl_real[b]) return;
    const float e = step_pos_normal(p, idx, b, rs.seed, l, 9u);
    const float cc = ci.cc[idx], sd = ci.std[idx];
    p.xt[idx] = noised ? fixed_noised_pos(ci.tab[l], ci.tab[T + l], ci.x0c[idx], cc, e, sd) : __fadd_rn(cc, __fmul_rn(e, sd));
  }
}
int launch_chain_init(const StepRowsArgs& rb, const StepRowsArgs& rv, const StepPosArgs& p, const ChainInitArgs& ci, hipStream_t st) {
  if (rb.NC != DD_NUM_B) return DD_ERR_UNSUPPORTED_SHAPE;
  return for_atom_classes(rv.NC, false, [&](auto nv, auto) -> int {
    if ((ci.mode != DD_INIT_PRIOR && ci.mode != DD_INIT_NOISED) || ci.cc == nullptr || ci.std == nullptr) return DD_ERR_BAD_ARG;
    if (ci.mode == DD_INIT_NOISED && (!ci.x0c || !ci.v0 || !ci.b0 || !ci.tab)) return DD_ERR_BAD_ARG;
    const int nb_b = (rb.rows + 3) / 4, nb_v = (rv.rows + 3) / 4, nb_p = (p.B * p.NL * 3 + 255) / 256;
    hipLaunchKernelGGL(k_chain_init<nv()>, dim3(nb_b + nb_v + nb_p), dim3(256), 0, st, rb, rv, p, ci, nb_b, nb_v);
    DD_CHECK_LAUNCH();
    return DD_OK;
  });
}

int launch_step_rows(const StepRowsArgs& a, hipStream_t st) {
  if (a.rows <= 0) return DD_OK;
  auto launch = [&](auto nc, auto fixed) -> int {
    hipLaunchKernelGGL((k_step_rows<nc(), fixed()>), dim3((a.rows + 3) / 4), dim3(256), 0, st, a);
    DD_CHECK_LAUNCH();
    return DD_OK;
  };
  const bool fixed = a.fx_mask != nullptr;
  return a.NC == DD_NUM_B ? with_fixed<DD_NUM_B>(fixed, launch) : for_atom_classes(a.NC, fixed, launch);
}
int launch_step_pos(const StepPosArgs& a, hipStream_t st) {
  const dim3 grid((a.B * a.NL * 3 + 255) / 256);
  if (a.fx_mask != nullptr) hipLaunchKernelGGL(k_step_pos<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_step_pos<false>, grid, dim3(256), 0, st, a);
  DD_CHECK_LAUNCH();
  return DD_OK;
}
int launch_reset_run_state(int32_t* rs, int t_start, uint64_t seed, hipStream_t st) {
  hipLaunchKernelGGL(k_reset_run_state, dim3(1), dim3(1), 0, st, rs, t_start, (uint32_t)seed, (uint32_t)(seed >> 32));
  DD_CHECK_LAUNCH();
  return DD_OK;
}
int launch_advance(int32_t* ctr, hipStream_t st) {
  hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, st, ctr);
  DD_CHECK_LAUNCH();
  return DD_OK;
}

}  // namespace dd

namespace dd {
// kind: stream id in the low byte (1 / 3 / 5 atom types, 2 / 4 / 6 bond types, 7 / 8 / 9 coordinates), atom class count in bits 8-15 (0 = 8)
template <int NC>
__device__ __forceinline__ void debug_uniforms(uint64_t seed, int step, long rows, uint32_t sid, long i, float* __restrict__ out) {
  if (i >= rows * NC) return;
  out[i] = philox_uniform<NC>(seed, i / NC, step, sid, (int)(i % NC));
}
__global__ __launch_bounds__(256) void k_debug_philox(uint64_t seed, int step, long rows, int kind, float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const uint32_t sid = (uint32_t)kind & 0xffu;
  const int nc = kind >> 8;
  if (sid == 7u || sid == 8u || sid == 9u) { if (i < rows) out[i] = philox_normal(seed, (int)i, step, sid); return; }
  if (sid == 2u || sid == 4u || sid == 6u) debug_uniforms<DD_NUM_B>(seed, step, rows, sid, i, out);
  else if (nc == 13) debug_uniforms<13>(seed, step, rows, sid, i, out);
  else if (nc == 23) debug_uniforms<23>(seed, step, rows, sid, i, out);
  else debug_uniforms<DD_NUM_V>(seed, step, rows, sid, i, out);
}
int launch_drift_armsca(const float* lig_pos, const int32_t* decomp_index, int B, int NL, float min_d, float max_d,
                        float* grad, int accumulate, int norm_B, hipStream_t st) {
  hipLaunchKernelGGL(k_drift_armsca, dim3(B), dim3(NL > 64 ? 128 : 64), 0, st, lig_pos, decomp_index, B, NL, min_d, max_d, grad, accumulate,
                     norm_B > 0 ? norm_B : B);
  DD_CHECK_LAUNCH();
  return DD_OK;
}
}  // namespace dd

extern "C" int dd_drift_armsca(const float* lig_pos, const int32_t* decomp_index, int B, int NL, float min_d,
                               float max_d, float* grad, int accumulate, void* stream) {
  if (!lig_pos || !decomp_index || !grad || B <= 0 || NL <= 0) return DD_ERR_BAD_ARG;
  if (NL > DD_NL_MAX) return DD_ERR_UNSUPPORTED_SHAPE;
  return dd::launch_drift_armsca(lig_pos, decomp_index, B, NL, min_d, max_d, grad, accumulate, B, (hipStream_t)stream);
}

namespace dd {
int launch_drift_arms_repul(const float* lig_pos, const int32_t* decomp_index, int B, int NL, float max_d, int mode, float* grad,
                            int accumulate, int norm_B, hipStream_t st) {
  hipLaunchKernelGGL(k_drift_arms_repul, dim3(B), dim3(DD_NL_MAX), 0, st, lig_pos, decomp_index, B, NL, max_d, mode, grad, accumulate,
                     norm_B > 0 ? norm_B : B);
  DD_CHECK_LAUNCH();
  return DD_OK;
}
}  // namespace dd

extern "C" int dd_drift_arms_repul(const float* lig_pos, const int32_t* decomp_index, int B, int NL, float max_d, int mode,
                                   float* grad, int accumulate, void* stream) {
  if (!lig_pos || !decomp_index || !grad || B <= 0 || NL <= 0 || (mode != 1 && mode != 2)) return DD_ERR_BAD_ARG;
  if (NL > DD_NL_MAX) return DD_ERR_UNSUPPORTED_SHAPE;
  return dd::launch_drift_arms_repul(lig_pos, decomp_index, B, NL, max_d, mode, grad, accumulate, B, (hipStream_t)stream);
}

namespace dd {
int launch_drift_clash(const float* lig_pos, const float* offset, const float* full_protein_pos, int B, int NL, int NF,
                       float sigma, float gamma, float* grad, int accumulate, const int32_t* nl_real, hipStream_t st) {
  hipLaunchKernelGGL(k_drift_clash, dim3(B * NL), dim3(256), 0, st, lig_pos, offset, full_protein_pos, B, NL, NF, sigma, gamma,
                     grad, accumulate, nl_real);
  DD_CHECK_LAUNCH();
  return DD_OK;
}
}  // namespace dd

extern "C" int dd_drift_clash(const float* lig_pos, const float* offset, const float* full_protein_pos, int B, int NL,
                              int NF, float sigma, float gamma, float* grad, int accumulate, void* stream) {
  if (!lig_pos || !offset || !full_protein_pos || !grad || B <= 0 || NL <= 0 || NF <= 0) return DD_ERR_BAD_ARG;
  return dd::launch_drift_clash(lig_pos, offset, full_protein_pos, B, NL, NF, sigma, gamma, grad, accumulate, nullptr,
                                (hipStream_t)stream);
}

// The caller's dd_restraints as a checked copy (fields beyond its `size` are NULL / 0) laid into the kernel's arguments: the point
// form first, then the trailing fields of the general form; `general` says whether any trailing array or trajectory pointer is set
// (none: everything behind it stays NULL / 0).  What the host can see is checked here; check_contents adds what only the device
// arrays say (synchronous copies on `st`, for the entry points that are called outside a capture).
namespace dd {
int read_restraints(const dd_restraints* rs, int B, int NL, bool has_decomp, bool has_v, bool check_contents, hipStream_t st,
                    RestraintArgs* out) {
  memset(out, 0, sizeof(*out));
  dd_restraints r;
  if (!read_sized(rs, &r)) return DD_ERR_BAD_ARG;
  if (B <= 0 || NL <= 0 || NL > DD_NL_MAX || r.R < 0 || !r.ptr || r.t_min > r.t_max) return DD_ERR_BAD_ARG;
  if (r.R > 0 && (!r.point || !r.min_d || !r.max_d || !r.weight || !r.atom || !r.group)) return DD_ERR_BAD_ARG;
  out->B = B; out->NL = NL; out->R = r.R; out->ptr = r.ptr; out->point = r.point; out->min_d = r.min_d; out->max_d = r.max_d;
  out->weight = r.weight; out->atom = r.atom; out->group = r.group; out->t_min = r.t_min; out->t_max = r.t_max; out->scale = r.scale != 0;
  const size_t R = (size_t)r.R;
  if (check_contents) {
    std::vector<int32_t> h((size_t)B + 1 + 2 * R);
    auto fetch = [&](int32_t* dst, const int32_t* src, size_t n) {       // (n ints to the host, waited for)
      return n == 0 || (hipMemcpyAsync(dst, src, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st) == hipSuccess &&
                        hipStreamSynchronize(st) == hipSuccess);
    };
    if (!fetch(h.data(), r.ptr, (size_t)B + 1)) { (void)hipGetLastError(); return DD_ERR_HIP; }
    if (h[0] != 0 || h[B] != r.R) return DD_ERR_BAD_ARG;                 // (before anything of length R is read)
    for (int b = 0; b < B; ++b)
      if (h[b + 1] < h[b]) return DD_ERR_BAD_ARG;
    if (!fetch(h.data() + B + 1, r.atom, R) || !fetch(h.data() + B + 1 + R, r.group, R)) {
      (void)hipGetLastError();
      return DD_ERR_HIP;
    }
    for (size_t i = 0; i < R; ++i) {
      const int at = h[B + 1 + i], gp = h[B + 1 + R + i];
      if (at < -1 || at >= NL) return DD_ERR_BAD_ARG;
      if (at == -1 && gp != DD_RESTRAINT_ANY && (gp < -1 || !has_decomp)) return DD_ERR_BAD_ARG;
    }
  }
  const bool traj = r.dist_traj || r.winner_traj || r.winner2_traj;
  out->general = r.cls || r.cls2 || r.pair || r.atom2 || r.group2 || r.form || traj;
  if (!out->general) return DD_OK;
  if ((r.cls || r.cls2) && !has_v) return DD_ERR_BAD_ARG;
  if (r.pair && !r.atom2 && !r.group2) return DD_ERR_BAD_ARG;
  if (traj && r.traj_positions <= 0) return DD_ERR_BAD_ARG;
  out->cls = r.cls; out->cls2 = r.cls2; out->pair = r.pair; out->atom2 = r.atom2; out->group2 = r.group2; out->form = r.form;
  out->dist_traj = r.dist_traj; out->winner_traj = r.winner_traj; out->winner2_traj = r.winner2_traj;
  out->traj_positions = traj ? r.traj_positions : 0;
  if (!check_contents || R == 0) return DD_OK;
  std::vector<int32_t> h(4 * R, 0);
  int32_t *pr = h.data(), *a2 = pr + R, *g2 = a2 + R, *fm = g2 + R;
  for (size_t i = 0; i < R; ++i) { a2[i] = -1; g2[i] = DD_RESTRAINT_NONE; }
  const int32_t* src[4] = {r.pair, r.atom2, r.group2, r.form};
  bool copied = true;
  for (int k = 0; k < 4; ++k)
    if (src[k] != nullptr) copied = copied && hipMemcpyAsync(h.data() + k * R, src[k], sizeof(int32_t) * R, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (!copied || hipStreamSynchronize(st) != hipSuccess) {              // (one wait for the copies that were issued)
    (void)hipGetLastError();
    return DD_ERR_HIP;
  }
  for (size_t i = 0; i < R; ++i) {
    if (fm[i] != 0 && fm[i] != 1) return DD_ERR_BAD_ARG;
    if (a2[i] < -1 || a2[i] >= NL) return DD_ERR_BAD_ARG;
    if (pr[i] != 0 && a2[i] == -1 && g2[i] != DD_RESTRAINT_ANY && (g2[i] < -1 || !has_decomp)) return DD_ERR_BAD_ARG;
  }
  return DD_OK;
}
}  // namespace dd

extern "C" int dd_drift_restraint2(const float* lig_pos, const int32_t* lig_v, const int32_t* decomp_index, const int32_t* nl_real, int B,
                                   int NL, const dd_restraints* restraints, const int32_t* step_counter, float* grad, int accumulate,
                                   float* dist, int32_t* winner, int32_t* winner2, void* stream) {
  if (!lig_pos || !grad || !restraints) return DD_ERR_BAD_ARG;
  dd::RestraintArgs a;
  const int rc = dd::read_restraints(restraints, B, NL, decomp_index != nullptr, lig_v != nullptr, true, (hipStream_t)stream, &a);
  if (rc != DD_OK) return rc;
  a.pos = lig_pos; a.decomp = decomp_index; a.nl_real = nl_real; a.step_counter = step_counter; a.grad = grad;
  a.accumulate = accumulate; a.dist = dist; a.winner = winner;
  a.lig_v = lig_v; a.winner2 = winner2;
  if (!a.general && winner2 != nullptr && a.R > 0 &&                    // (the point kernel knows no second winner: all -1)
      hipMemsetAsync(winner2, 0xff, sizeof(int32_t) * (size_t)a.R, (hipStream_t)stream) != hipSuccess) {
    (void)hipGetLastError();
    return DD_ERR_HIP;
  }
  return dd::launch_drift_restraint(a, (hipStream_t)stream);
}

extern "C" int dd_drift_restraint(const float* lig_pos, const int32_t* decomp_index, const int32_t* nl_real, int B, int NL,
                                  const dd_restraints* restraints, const int32_t* step_counter, float* grad, int accumulate, float* dist,
                                  int32_t* winner, void* stream) {
  if (!lig_pos || !grad || !restraints) return DD_ERR_BAD_ARG;
  dd::RestraintArgs a;
  const int rc = dd::read_restraints(restraints, B, NL, decomp_index != nullptr, false, true, (hipStream_t)stream, &a);
  if (rc != DD_OK) return rc;
  if (a.general) return DD_ERR_BAD_ARG;                                  // (the general form has its own entry point)
  a.pos = lig_pos; a.decomp = decomp_index; a.nl_real = nl_real; a.step_counter = step_counter; a.grad = grad;
  a.accumulate = accumulate; a.dist = dist; a.winner = winner;
  return dd::launch_drift_restraint(a, (hipStream_t)stream);
}

// Test aid: the production noise of one step, exactly as the step kernels draw it.  kind (low byte) 1: uniforms [rows,8] of the
// atom-type stream, 2: uniforms [rows,5] of the bond-type stream, 7: normals [rows] of the coordinate stream; 3 / 4 / 8: the same
// three of a resampling jump (`step` is the Philox time word, t + 65536 * epoch); 5 / 6 / 9: the same three of the chain init
// (dd_chain_init; `step` is the level drawn).  Bits 8-15 of kind: the atom class count of kinds 1 / 3 / 5 (0 or 8, 13, 23 ->
// [rows, that many]).
extern "C" int dd_debug_philox(uint64_t seed, int step, long rows, int kind, float* out, void* stream) {
  const int sid = kind & 0xff, nc = kind >> 8;
  const bool atoms = sid == 1 || sid == 3 || sid == 5, bonds = sid == 2 || sid == 4 || sid == 6, normals = sid == 7 || sid == 8 || sid == 9;
  if (!out || rows <= 0 || kind < 0 || !(atoms || bonds || normals)) return DD_ERR_BAD_ARG;
  if (nc != 0 && (!atoms || (nc != 8 && nc != 13 && nc != 23))) return DD_ERR_BAD_ARG;
  const long n = normals ? rows : rows * (atoms ? (nc ? nc : DD_NUM_V) : DD_NUM_B);
  hipLaunchKernelGGL(dd::k_debug_philox, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, step, rows, kind, out);
  DD_CHECK_LAUNCH();
  return DD_OK;
}
