// Kernel argument structs and launcher prototypes shared by the translation units.
#pragma once
#include <string.h>

#include "dd_common.hpp"

namespace dd {

// A checked copy of a caller's `size`-prefixed struct (include/decompdiff_hip.h: dd_fixed, dd_resample, dd_init, dd_restraints):
// fields beyond the caller's `size` read as NULL / 0, so a caller built against a shorter struct keeps working; the copy's `size`
// is the full one.  false (and all zeros): NULL, or a size outside [4, 4096].
template <class T>
inline bool read_sized(const T* in, T* out) {
  memset(out, 0, sizeof(T));
  if (in == nullptr || in->size < (int32_t)sizeof(int32_t) || in->size > 4096) return false;
  memcpy(out, in, (size_t)in->size < sizeof(T) ? (size_t)in->size : sizeof(T));
  out->size = (int32_t)sizeof(T);
  return true;
}

struct FlagWait { const int32_t* flags; int idx0, n0, idx1, n1; };       // up to two counters (idx < 0: none)
inline FlagWait no_wait() { return FlagWait{nullptr, -1, 0, -1, 0}; }

struct GemmArgs {
  const float* X; int x_rows_per_b; long x_stride_b; int ldx; int rows;
  const float* W; const float* bias; const float* ln;
  float* Y; int y_rows_per_b; long y_stride_b; int ldy; int ncols; int accumulate;
  // optional second addend for X rows that are ligand nodes: X[b*N + n] += X2[b*NL + n - NP] (n >= NP)
  const float* X2; int x2_N, x2_NP;
  // x2_Eb > 0 selects the other addend form: X row r is a bond edge, X2 row = its destination atom
  //   X[r] += X2[((r / x2_Eb) * x2_N + (r % x2_Eb) / x2_NLm1) * x2_ld]      (x2_N = ligand atoms per sample here)
  int x2_Eb, x2_NLm1, x2_ld;
  long long* dbg;          // profiling aid: s_memtime phase stamps, 8 per workgroup (single launches only)
  const float* acc_src;    // accumulate = 1: the addend is read from acc_src (same layout as Y) instead of Y itself (NULL: Y)
};
inline GemmArgs gemm_args(const float* X, int x_rows_per_b, long x_stride_b, int ldx, int rows, const float* W,
                          const float* bias, const float* ln, float* Y, int y_rows_per_b, long y_stride_b, int ldy,
                          int ncols, int accumulate) {
  GemmArgs g{X, x_rows_per_b, x_stride_b, ldx, rows, W, bias, ln, Y, y_rows_per_b, y_stride_b, ldy, ncols, accumulate,
             nullptr, 0, 0, 0, 0, 0, nullptr, nullptr};
  return g;
}
// Persistent layer-tail queue (dd_gemm.hip::k_gemm_tail): jobs in dependency order, counters in the workspace.
// Flag words (int32, zeroed by the first launch of every forward), per layer DD_FLAGS_PER_LAYER of them, EACH ON ITS OWN
// 128-byte line (DD_FLAG_STRIDE ints apart): agent-scope atomics on one word retire at ~12 ns each device-wide
// (tools/bench_atomics.hip) and every poll of a word on the same line queues with them -- with all of a layer's words in
// one line the queue took 330 us instead of 40.
enum { DD_FLAG_TICKET = 0, DD_FLAG_LIN = 1, DD_FLAG_TICKET2 = 2, DD_FLAG_PL1 = 3, DD_FLAG_P1Q = 4, DD_FLAG_PBQ = 5, DD_FLAG_PB1R = 6,
       DD_FLAG_NODE = 7, DD_FLAGS_PER_LAYER = 8 };
constexpr int DD_FLAG_LAYERS = 8;
constexpr int DD_FLAG_STRIDE = 32;
constexpr int DD_FLAG_ERR = DD_FLAG_LAYERS * DD_FLAGS_PER_LAYER * DD_FLAG_STRIDE;   // first spin that timed out (0 = none); sticky
#if defined(DD_DEBUG_OPTIONS) && DD_DEBUG_OPTIONS
constexpr int DD_NUM_FLAGS = DD_FLAG_ERR + DD_FLAG_STRIDE;
#else
constexpr int DD_NUM_FLAGS = 0;                                         // the default library's workspace carries no flag words
#endif
constexpr int DD_NUM_COUNTERS = 192;                                    // [0, 64): work counters of the persistent attention workgroups (per
                                                                        // layer), [64, 128): tile counters of the coordinate launches (k_attn2_pos_g), [128, 192): block counters of the persistent
                                                                        // node_layer_with_edge workgroups (two per layer: protein / ligand centres)
constexpr int DD_TAIL_CHUNK = 2;                                        // consecutive tiles drawn per ticket
constexpr int DD_TAIL_MAX_JOBS = 14;
struct TailJob {
  GemmArgs g;
  int nbx, tiles;                        // filled by launch_gemm_tail
  int wait0, wait0_n, wait1, wait1_n;    // flag index (-1: none) that must have reached the target before a tile starts
  int sig;                               // flag index bumped by every finished tile (-1: none)
};
struct TailArgs {
  TailJob job[DD_TAIL_MAX_JOBS];
  int end[DD_TAIL_MAX_JOBS];             // cumulative tile counts
  int njobs, total, ticket, persist;     // ticket: index of this launch's ticket counter; persist: workgroups loop over tickets
  int32_t* flags;
};
inline TailJob tail_job(const GemmArgs& g, int wait0 = -1, int wait0_n = 0, int sig = -1, int wait1 = -1, int wait1_n = 0) {
  TailJob q{g, 0, 0, wait0, wait0_n, wait1, wait1_n, sig};
  return q;
}
inline int gemm_tiles(int rows, int cols) { return ((rows + 63) / 64) * ((cols + 63) / 64); }
int launch_gemm_tail(TailArgs& ta, hipStream_t st);
int launch_gemm128(const GemmArgs& a, hipStream_t st);
// up to 6 independent projections in one launch (small ones ride along with the big ones)
int launch_gemm128_batch(const GemmArgs* jobs, int njobs, hipStream_t st);
// node output MLPs + lin_node of a layer (x2h_out_fc; dd_node_out.hip): out = h + W2_e' z_e + W2_b' z_b + c0 over all B (NP + NL)
// rows; Ab holds the ligand rows only ([B, NL, 128]); blk: the layer's weight block (DD_NO_* offsets); out may be h
struct NodeOutArgs { const float* Ae; const float* Ab; const float* h; float* out; const float* blk; int B, NP, NL; };
int launch_node_out_fc(const NodeOutArgs& a, hipStream_t st);

// ---- head of a forward, block boundaries and the bond-layer assemble (dd_graph.hip); built by dd_api.hip::Fwd
// One kNN + edge-weight problem: B samples of NP protein + NL ligand atoms (an op-level [B, N, 3] tensor: NP = N, NL = 0).
struct GraphArgs {
  int B, NP, NL, K;
  // positions: the first protein row and the first ligand row of sample 0, each with its per-sample stride in floats --
  // the sampler's separate buffers (protein_pos, 3 NP) and (lig_pos, 3 NL), or one [B, N, 3] block (set_block)
  const float* prot; int prot_stride;
  const float* lig; int lig_stride;
  int32_t* nbr;            // [B,N,K]
  float* ew;               // [B,N,K] (launch_knn: unused)
  const float *EW_W1T, *EW_b1, *EW_ln, *EW_w2, *EW_b2;   // edge-weight MLP (launch_knn: unused)
  // padded heterogeneous batches: padding atoms are neither centres nor candidates (NULL: dense batch)
  const int32_t *np_real, *nl_real;
  void set_block(const float* x) { prot = x; lig = x + 3 * (long)NP; prot_stride = lig_stride = 3 * (NP + NL); }
};
int launch_graph(const GraphArgs& a, hipStream_t st);              // kNN + edge weights in one launch, the list handed over through LDS
// the two halves as launches of their own (edge weights: of the lists in nbr): positions in one [B, N, 3] block only
int launch_knn(const GraphArgs& a, hipStream_t st);
int launch_edge_weights(const GraphArgs& a, hipStream_t st);

// Embeddings / context: 256-thread blocks [0, node_blocks) write one float of h each (+ the workspace copies of x_t), blocks
// [node_blocks, blocks) one float of h_bond; block 0 also zeroes the work counters and advances the step index.
struct EmbedArgs {
  int B, NP, NL;
  int nv;                   // atom classes (columns of the ligand embedding before the two indicators)
  // inputs: sampler state and embedding weights
  const float *protein_h, *protein_pos, *lig_pos;
  const int32_t* lig_v;
  const float* lig_aux;
  const int32_t* bond;
  const float *Wl, *bl, *Wb, *bb;
  // outputs: h, both copies of x, h_bond
  float *h, *xa, *xb, *hb;
  int32_t *counters, *advance;   // (either may be NULL)
  long bond_rows;           // B NL (NL - 1)
  int node_blocks, blocks;
};
// Layer-0 rows of the ligand atoms / bonds gathered from dd_sampler.l0_tables (see include/decompdiff_hip.h): one thread per
// float4, the atoms' [0, atom_f4) in front of the bonds'
constexpr int l0_atom_f4(int pl_width) { return 160 + pl_width / 4 + 32 + 32; }   // float4 per atom: 640 + PL row + 128 + 128 floats
constexpr int DD_L0_ATOM_F4 = l0_atom_f4(1280);
constexpr int DD_L0_BOND_F4 = 160 + 32;              // float4 per bond: 640 + 128 floats
struct Layer0RowsArgs {
  int B, NP, NL;
  const float* tab;
  const int32_t* lig_v;
  const float* lig_aux;
  const int32_t* bond;
  float *l0_P, *PL, *l0_qn, *qlnb, *PB, *qb;
  long atom_f4;            // B NL l0_atom_f4(pl_width)
  int blocks;
  int pl_width;            // floats of a PL row gathered: 1280, or 640 for the narrow bond layer (the row stride stays 1280)
};
int launch_embed(const EmbedArgs& e, hipStream_t st);
int launch_layer0_rows(const Layer0RowsArgs& r, hipStream_t st);
int launch_head_rows(const EmbedArgs& e, const Layer0RowsArgs* r /*NULL: no tables*/, hipStream_t st);   // both, one launch

// Host-side arguments of the bond-layer assemble launch (k_bl_assemble3 takes them one by one)
struct AssembleArgs {
  const float *x, *PB, *PL, *Wgp;
  int B, NP, NL;
  float *Ek, *Ev, *q1, *Rk, *Rv;   // (q1 may be NULL: the query GEMM sums its hidden rows itself)
  // deferred coordinate update of the previous layer (xprev != NULL): xout = xprev + dxe + dxb on the ligand rows
  const float *xprev, *dxe, *dxb;
  float* xout;
  FlagWait fw;              // PB / PL produced by the layer-tail queue (measurement build)
  bool narrow;              // narrow bond layer (h_node_in_bond_net: False): PL is not read, q1 must be NULL
};
int launch_bl_assemble(const AssembleArgs& a, hipStream_t st);
int launch_drift_armsca(const float* lig_pos, const int32_t* decomp_index, int B, int NL, float min_d, float max_d,
                        float* grad, int accumulate, int norm_B, hipStream_t st);
int launch_drift_arms_repul(const float* lig_pos, const int32_t* decomp_index, int B, int NL, float max_d, int mode, float* grad,
                            int accumulate, int norm_B, hipStream_t st);
// (nl_real: padded heterogeneous batches -- padding atoms are neither centres nor candidates)
int launch_drift_clash(const float* lig_pos, const float* offset, const float* full_protein_pos, int B, int NL, int NF,
                       float sigma, float gamma, float* grad, int accumulate, const int32_t* nl_real, hipStream_t st);
// Distance restraints (include/decompdiff_hip.h, dd_restraints): gradient of sum_r w_r (relu(min_d_r - d_r) + relu(d_r - max_d_r)),
// d_r the distance of the point to the explicit atom or to the first nearest member of the group.  Every pointer is a DEVICE
// pointer read at launch; R bounds what ptr may address.  step_counter != NULL: the term acts only while t_min <= t <= t_max
// (t = run state's t_start - (steps done - counter_bias)) and writes zeros outside.
struct RestraintArgs {
  const float* pos;              // [B*NL,3] centred ligand coordinates
  const int32_t* decomp;         // [B*NL] arm ids (-1 scaffold, -2 padding) or NULL: arm / scaffold groups are empty
  const int32_t* nl_real;        // [B] real ligand sizes of a padded batch or NULL
  int B, NL, R;
  const int32_t* ptr;            // [B+1] CSR: restraints ptr[b] .. ptr[b+1] belong to sample b
  const float *point, *min_d, *max_d, *weight;   // [R,3], [R], [R], [R]; points in the frame of pos
  const int32_t *atom, *group;   // [R] row within the sample or -1: the group (DD_RESTRAINT_ANY, -1 scaffold, >= 0 arm id)
  const int32_t* step_counter;   // run state [4] or NULL: always active
  int counter_bias, t_min, t_max;
  int scale;                     // (host side only: the step multiplies the gradient by tab_score[t])
  float* grad;                  // [B*NL,3], every row written
  int accumulate;
  float* dist;                   // [R] or NULL
  int32_t* winner;               // [R] row within the sample or -1, or NULL
  // The general form (dd_restraints' trailing fields): class masks over the current atom classes, ligand-ligand pairs, harmonic
  // hinges and per-step rows of dist / winner(s).  `general`: the caller's struct carries a non-NULL trailing array -- the launch
  // takes k_drift_restraint<true> --, else everything below is NULL / 0 and the point instantiation reads none of it.
  bool general;
  const int32_t* lig_v;          // [B*NL] current atom classes or NULL (then cls / cls2 are NULL too)
  const uint32_t *cls, *cls2;    // [R] class masks (bit c = class c) or NULL: untyped
  const int32_t *pair, *atom2, *group2, *form;   // [R] each or NULL: no pairs / no explicit second atom / no second group / linear
  int32_t* winner2;              // [R] the j of a pair (row within the sample) or -1, or NULL
  float* dist_traj;              // [traj_positions, R] or NULL; row = the run state's step
  int32_t *winner_traj, *winner2_traj;
  int traj_positions;
};
int launch_drift_restraint(const RestraintArgs& a, hipStream_t st);   // (picks the instantiation from a.general)
// the caller's dd_restraints, checked, as the kernel's arguments (pos / decomp / nl_real / lig_v / step_counter / outputs left to the
// caller); has_v: the caller has atom classes for cls / cls2; check_contents: also what only the device arrays say -- copies
// ptr / atom / group (and pair / atom2 / group2 / form) to the host and waits for `st`
int read_restraints(const dd_restraints* rs, int B, int NL, bool has_decomp, bool has_v, bool check_contents, hipStream_t st,
                    RestraintArgs* out);
int launch_extract_ligand(const float* x, int B, int NP, int NL, float* out, hipStream_t st);

enum { M_NE = 0, M_NB = 1, M_BL = 2, M_PE = 3, M_PB = 4 };

struct AttnArgs {
  int B, NP, NL, K;
  const float* x;          // [B,N,3] positions at layer input
  const int32_t* nbr;      // [B,N,K]
  const float* ew;         // [B,N,K]
  const float *kd, *ks, *vd, *vs, *ke, *ve;   // projection tables
  int ld_kd, ld_ks, ld_vd, ld_vs, ld_ke, ld_ve;
  const float* q;          // [segments,128]
  const float *Akp, *Avp;  // [4,24,128] MFMA A-operand layout (tiled kernel)
  const float *Wakp, *Wavp; // [12,128] merged angle-code columns (BL, tiled kernel)
  const float *lnk, *lnv;  // [2,128]
  const float* W2k;        // [128,128]
  const float* b2v;        // node modes
  const float* W2v;        // node modes, tiled kernel: [128 o][128 c]
  // coordinate modes, optional: second layer of the query MLP evaluated in the kernel (q is then ignored)
  const float *qhid, *lnq, *W2q, *b2q; int ld_qhid;   // hidden pre-activation rows [B*NL, ld_qhid], LN [2,128], W2q^T [128 k,128 o], [128]
  int* work_counter;       // persistent workgroups: next segment to process (zeroed before the launch)
  const float *W2v16, *b2v16;  // pos modes
  float* out;
  const float* dxe;        // PB: result of PE
  float* x_next;           // PB
  const float *Rk, *Rv;    // BL (tiled kernel): per-edge G(d_ji) partial sums [B*Eb,128]
  long long* dbg_clock;    // optional [n_blocks][16] s_memtime stamps of wave 0 (profiling aid), may be NULL
  int out_assign;          // NB: 1 = write (=) rows [B*NL,128] of `out` instead of accumulating into the node table
  // padded heterogeneous batches (dd_sampler.np_real / nl_real / bl_prefix), all NULL for dense batches
  const int32_t *np_real, *nl_real, *bl_prefix;
  // inputs produced by the layer-tail queue running on the other stream (dd_gemm.hip::k_gemm_tail): the launch starts
  // without a graph edge and polls flags[wait_idx] >= wait_n before its first read of them (NULL: ordinary stream order)
  const int32_t* wait_flags; int wait_idx, wait_n;
  // persistent bond-layer workgroups: work_counter hands out TRIPS.  Trips t < trip_full cover NW consecutive segments each
  // (whole rounds of all persistent workgroups); the remainder -- less than one round -- is spread evenly: trip t >= trip_full
  // covers trip_q (< NW) segments, so that the last round runs one wave per SIMD on every CU instead of full trips on some CUs
  // beside idle ones.  Set by launch_attn2_node (trip_q = 0 and trip_full = 1 << 27: plain NW-segment trips).
  int trip_full, trip_q;
  // lin_node inside the node launch (NE / NB blocks, fused launch only; NULL: the attention output goes to `out` as before):
  //   NE: out[row] += W_lin . A[row] + lin_b (+ lin_add[ligand row]: the previous layer's W_lin . A_nb, still pending) -- `out` = h;
  //   NB: out[ligand row] = W_lin . A_nb[row]   (W_lin [128 o][128 c], models/encoders/uni_transformer_edge.py:276-277)
  const float *lin_W, *lin_b, *lin_add;
};

int launch_attn2(int mode, const AttnArgs& a, hipStream_t st);   // one sub-layer: 16-member tiles, scores/aggregation on MFMA
int launch_attn2_node(const AttnArgs& ne, const AttnArgs& nb, const AttnArgs& bl, hipStream_t st);   // NE+NB+BL, one launch (ne.wait_*)
int launch_attn2_pos(const AttnArgs& pe, const AttnArgs& pb, hipStream_t st);                        // PE+PB, one launch
// ... with the projections that feed it computed by its leading workgroups (dd_attention2.hip::k_attn2_pos_g)
int launch_attn2_pos_g(const AttnArgs& pe, const AttnArgs& pb, const GemmArgs* jobs, int njobs, int n_lead, int32_t* counter,
                       hipStream_t st);
int launch_xupdate(const float* x, const float* dxe, const float* dxb, int B, int NP, int NL, float* x_next, hipStream_t st);

struct StepRowsArgs {
  const float* hid;        // [rows,128] first Linear of the head (pre-activation incl. bias)
  const float* logits_in;  // [rows,NC] head outputs supplied by the host instead of hid / W2 / b2 (dd_reverse_step: k_step_rows of a
                           // chain without fixed atoms reads them; k_step_all never does), or NULL
  const float* W2;         // [NC,128]
  const float* b2;         // [NC]
  int rows, NC, rows_per_sample;
  const float* tab;        // [4][T] log_alphas, log_1m_alphas, log_cumprod, log_1m_cumprod, then [NC] log prior
  int T;
  const int32_t* step_counter;   // run state [4]: steps done, t_start, seed lo, seed hi (dd_sampler_reset)
  int counter_bias;        // step index = step_counter[0] - counter_bias (1 when the forward's first launch advanced it)
  int32_t* state;          // [rows] current class, updated in place
  const float* uniforms;   // [n_steps, rows, NC] or NULL
  uint32_t stream_id;
  float* logits_out;       // [rows,NC] raw logits (pred_*), may be NULL
  float* traj_recon;       // [n_steps, rows, NC] log_softmax(logits), may be NULL
  float* traj_prob;        // [n_steps, rows, NC] posterior log-probs, may be NULL
  int32_t* traj_state;     // [n_steps, rows] sampled classes, may be NULL
  // per-sample noise keys (dd_sample_steps_keyed), NULL: the run state's seed and the flat row address the draws.
  // Not NULL: sample b = row / rows_per_sample draws with key sample_keys[b] at the row of its OWN dense enumeration --
  // atoms: the index in the sample; bonds: dst * (n - 1) + sp, n = nl_real[b] (padded batches) or NL.
  const uint64_t* sample_keys;   // [B], read at every launch
  const int32_t* nl_real;        // [B] real ligand sizes (bond rows of padded batches), or NULL
  int NL;                        // dense ligand width (bond rows: rows_per_sample = NL * (NL - 1))
  // fixed atoms (dd_sample_steps_fixed; include/decompdiff_hip.h), all device pointers read at every launch.  fx_mask == NULL:
  // nothing is held.  An atom row is held iff its mask byte is set, a bond row (fx_bond) iff both its endpoints' are.
  const uint8_t* fx_mask;        // [B*NL]
  const int32_t* fx_val;         // [rows] known clean classes (read at held rows only)
  int fx_mode;                   // DD_FIXED_HOLD / DD_FIXED_REPLACE
  int fx_bond;                   // 1: the rows are bond rows dst * (NL - 1) + sp of their sample
  // resampling (dd_resample; FIXED instantiations only): the chain's epoch, a device int read at every launch -- the Philox
  // time word of a step is t + 65536 * epoch.  NULL: epoch 0, today's draws.
  const int32_t* epoch;
};
struct StepPosArgs {
  int B, NL, T;
  const int32_t* step_counter;   // run state [4], see StepRowsArgs
  int counter_bias;
  const float* x0;          // [B*NL,3] predicted x0 (centred)
  // deferred tail of the forward: x0 = x0_prev[ligand rows] + x0_dxe + x0_dxb (the last layer's coordinate update,
  // same association as k_xupdate), also stored to x0_out; x0 is ignored then
  const float* x0_prev; const float* x0_dxe; const float* x0_dxb; float* x0_out; int NP;
  float* xt;                // [B*NL,3] current positions, updated in place
  const float* tab_pos;     // [3][T] c0, ct, logvar
  const float* tab_score;   // [T]
  const float* atom_std;    // [B*NL,3]
  const float* offset;      // [B,3]
  const float* grad_a; int scale_a;   // armsca gradient (may be NULL)
  const float* grad_c; int scale_c;   // clash gradient (may be NULL)
  const float* grad_r; int scale_r;   // arms_repul gradient (may be NULL)
  const float* grad_q; int scale_q;   // restraint gradient (may be NULL); the four are added in this order
  const float* eps;         // [n_steps,B*NL,3] or NULL
  float* traj_pos;          // [n_steps,B*NL,3] or NULL
  const uint64_t* sample_keys;   // [B] per-sample noise keys or NULL: key sample_keys[b], index 3 * i + c inside the sample
  // fixed atoms (see StepRowsArgs); fx_mask == NULL: nothing is held
  const uint8_t* fx_mask;        // [B*NL]
  const float* fx_x0c;           // [B*NL,3] known clean coordinates, centred
  const float* fx_cc;            // [B*NL,3] centred prior centres of the atoms' arms (replace mode)
  const float* fx_tab;           // [2][T] sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod) (replace mode)
  int fx_mode;
  const int32_t* epoch;          // resampling: the chain's epoch (see StepRowsArgs), or NULL
};
int launch_step_rows(const StepRowsArgs& a, hipStream_t st);
int launch_step_pos(const StepPosArgs& a, hipStream_t st);
int launch_advance(int32_t* ctr, hipStream_t st);
int launch_reset_run_state(int32_t* rs, int t_start, uint64_t seed, hipStream_t st);
int launch_step_all(const StepRowsArgs& rb, const StepRowsArgs& rv, const StepPosArgs& p, hipStream_t st);
// fixed atoms: hold mode writes the known values into the state, replace mode draws the held rows' level t_start (the run state's)
// at Philox time t_start + 1; atoms, bonds and coordinates in one launch
int launch_fixed_init(const StepRowsArgs& rb, const StepRowsArgs& rv, const StepPosArgs& p, hipStream_t st);
// resampling: the forward jump q(x_m | x_l), m = l + j, of every row that a jump moves (bond rows, atom rows, coordinates: one
// launch) with the coefficients jtab [6][T] at m, then a one-thread launch that rebases the run state (t_start += j) and bumps
// the epoch.  rb / rv / p as for a step of the chain (fixed atoms and the epoch pointer set).
int launch_jump(const StepRowsArgs& rb, const StepRowsArgs& rv, const StepPosArgs& p, const float* jtab, int j, int32_t* epoch,
                hipStream_t st);
int launch_reset_epoch(int32_t* epoch, hipStream_t st);
// chain init (dd_init): the chain's level in front of its first step for every real row -- bond rows, atom rows, coordinates: one
// launch.  rb / rv / p as for a step of the chain (sample_keys set for a keyed chain; no fixed atoms needed).
struct ChainInitArgs {
  int mode;                      // DD_INIT_PRIOR / DD_INIT_NOISED
  const float* cc;               // [B*NL,3] centred centres
  const float* std;              // [B*NL,3]
  const float* lp_v;             // [NC] log prior of the atom classes, or NULL: the chain's (tab_v[4 * T + c])
  const float* lp_b;             // [5] log prior of the bond classes, or NULL: the chain's
  const float* x0c;              // noised: [B*NL,3] clean centred coordinates
  const int32_t* v0;             // noised: [B*NL] clean atom classes
  const int32_t* b0;             // noised: [B*NL*(NL-1)] clean bond classes
  const float* tab;              // noised: [2][T] sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod)
  const int32_t* nl_real;        // [B] real ligand sizes of a padded batch (atom rows, coordinates), or NULL
};
int launch_chain_init(const StepRowsArgs& rb, const StepRowsArgs& rv, const StepPosArgs& p, const ChainInitArgs& ci, hipStream_t st);

}  // namespace dd
