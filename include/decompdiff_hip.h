/*
 * decompdiff_hip.h — C ABI of libdecompdiff_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the reverse-diffusion sampling hot path of bytedance/DecompDiff
 * (SURVEY.md §8b).  The reference is pure Python on PyTorch; the native ops its hot path
 * reaches live in third-party wheels (torch_scatter / torch_cluster / torch_sparse / ATen).
 * Each entry point below names the reference call site(s) it replaces.  All pointers are
 * DEVICE pointers unless marked HOST; the caller owns every buffer; nothing is allocated,
 * freed or synchronised inside (two documented exceptions: dd_sample_steps_graph waits for its
 * own replays before destroying the graph, dd_profile_step reads its events); every launch goes
 * to `stream` (a hipStream_t passed as void*).  Return value: 0 on success, negative dd_status on error (no exceptions cross
 * the ABI); dd_status_string() gives the text.
 *
 * Dense fixed-shape layout ("padded/masked fixed-size pocket+ligand graphs"):
 *   B samples; per sample NP protein atoms then NL ligand atoms (N = NP+NL, the context
 *   order of models/common.py:167-194); kNN lists [B,N,K]; the fully connected ligand bond
 *   graph is implicit and dst-major: edge e = dst*(NL-1) + src - (src>dst)
 *   (utils/transforms.py:331-337); triplets (k->j->i) are implicit (closed-form indices).
 */
#ifndef DECOMPDIFF_HIP_H
#define DECOMPDIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DD_HIDDEN 128
#define DD_HEADS 16
#define DD_NGAUSS 20
#define DD_KNN_MAX 64    /* neighbours per centre (kNN segments of up to 2 / 4 tiles of 16 members: K <= 32 / K <= 64) */
#define DD_NL_MAX 128     /* ligand atoms per sample supported by the fused kernels (tile counts 2 / 3 / 4 / 8 of 16 members) */
#define DD_N_MAX 2048     /* atoms per sample supported by the kNN kernel (candidates per lane: 2 / 4 / 6 / 11 / 16 / 32) */
#define DD_NUM_V 8        /* atom classes of ligand_atom_mode 'basic' (scripts/sample_diffusion_decomp.py:540); dd_sampler.num_v
                             selects 13 ('add_aromatic') or 23 ('full') instead (utils/transforms.py:15-64,138-151) */
#define DD_NUM_V_MAX 23
#define DD_NUM_B 5        /* bond classes  (configs/training.yml:33) */

typedef enum dd_status {
  DD_OK = 0,
  DD_ERR_BAD_ARG = -1,
  DD_ERR_UNSUPPORTED_SHAPE = -2,
  DD_ERR_WORKSPACE_TOO_SMALL = -3,
  DD_ERR_HIP = -4
} dd_status;

/* Packed-weight slots, per layer (decompdiff_amd/packing.py: LAYER_SLOTS, same order). */
typedef enum dd_wslot {
  DD_W_n1, DD_b_n1, DD_W_l1, DD_b_l1, DD_W_b1, DD_b_b1,
  DD_NE_Ak, DD_NE_Av, DD_NE_lnk, DD_NE_lnv, DD_NE_lnq, DD_NE_W2q, DD_NE_b2q, DD_NE_W2k, DD_NE_W2vT, DD_NE_b2v, DD_NE_W2v, DD_NE_Akp, DD_NE_Avp,
  DD_NB_lnk, DD_NB_lnv, DD_NB_lnq, DD_NB_W2q, DD_NB_b2q, DD_NB_W2k, DD_NB_W2vT, DD_NB_b2v, DD_NB_W2v,
  DD_BL_Wg1k, DD_BL_Wg1v, DD_BL_Wg2k, DD_BL_Wg2v, DD_BL_Wak, DD_BL_Wav,
  DD_BL_lnk, DD_BL_lnv, DD_BL_lnq, DD_BL_W2q, DD_BL_b2q, DD_BL_W2k, DD_BL_W2vT, DD_BL_b2v, DD_BL_W2v, DD_BL_Wgp, DD_BL_Wakp, DD_BL_Wavp,
  DD_W_lin, DD_b_lin,
  DD_W_n2, DD_b_n2, DD_W_l2, DD_b_l2, DD_W_b2, DD_b_b2,
  DD_PE_Ak, DD_PE_Av, DD_PE_lnk, DD_PE_lnv, DD_PE_lnq, DD_PE_W2q, DD_PE_b2q, DD_PE_W2k, DD_PE_W2v, DD_PE_b2v, DD_PE_Akp, DD_PE_Avp, DD_PE_W2qT,
  DD_PB_lnk, DD_PB_lnv, DD_PB_lnq, DD_PB_W2q, DD_PB_b2q, DD_PB_W2k, DD_PB_W2v, DD_PB_b2v, DD_PB_W2qT,
  DD_NUM_LAYER_SLOTS
} dd_wslot;

/* Global slots (packing.py: GLOBAL_SLOTS), stored after all layers. */
typedef enum dd_gslot {
  DD_G_W_pemb, DD_G_b_pemb, DD_G_W_lemb, DD_G_b_lemb, DD_G_W_bemb, DD_G_b_bemb,
  DD_G_EW_W1T, DD_G_EW_b1, DD_G_EW_ln, DD_G_EW_w2, DD_G_EW_b2,
  DD_G_VH_W1, DD_G_VH_b1, DD_G_VH_W2, DD_G_VH_b2,
  DD_G_BH_W1, DD_G_BH_b1, DD_G_BH_W2, DD_G_BH_b2,
  DD_NUM_GLOBAL_SLOTS
} dd_gslot;

/* One sampler run: everything `DecompScorePosNet3D.sample_diffusion`
 * (models/decompdiff.py:552-703) keeps alive across its loop. */
typedef struct dd_sampler {
  /* shapes */
  int32_t B, NP, NL, K, NF;        /* NF: full-protein atoms per sample (clash drift), 0 = none */
  int32_t num_layers;
  int32_t T;                       /* length of the schedule tables */
  int32_t t_start;                 /* timestep of step 0 (reference: num_timesteps-1) */
  /* model */
  const float* weights;            /* packed arena */
  const int64_t* slot_off;         /* HOST: offsets (floats) [num_layers*DD_NUM_LAYER_SLOTS + DD_NUM_GLOBAL_SLOTS].
                                      The table also says which bond layer the model has (h_node_in_bond_net of the reference's
                                      configuration): DD_b_l1 follows DD_W_l1, and (slot_off[DD_b_l1] - slot_off[DD_W_l1]) / 128 is
                                      1280 for the wide bond layer (True: W_l1 = node_layer_with_bond kd|ks|vd|vs|q1 and bond_layer
                                      k_hk|k_hj|v_hk|v_hj|q_hi) and 640 for the narrow one (False: the node_layer_with_bond blocks
                                      only; the bond layer's first Linears have no atom columns, and W_b1 holds their h_bond columns
                                      as before).  Every entry point that runs the network reads it once per call from every layer;
                                      any other value, or layers that disagree: DD_ERR_BAD_ARG. */
  const float* tab_pos;            /* [3][T]: coefficient of the network's coordinate output, coefficient of x_t, posterior_logvar.
                                      C0: posterior_mean_c0_coef, posterior_mean_ct_coef.  model_mean_type 'noise': the eps -> x0
                                      map folded in, -c0 * sqrt_recipm1_alphas_cumprod and ct + c0 * (sqrt_recip_alphas_cumprod +
                                      sqrt_recipm1_alphas_cumprod) (DecompScorePosNet3D.position_step_table) */
  const float* tab_v;              /* [4][T]: log_alphas_v, log_one_minus_alphas_v, log_alphas_cumprod_v, log_one_minus_alphas_cumprod_v (atoms),
                                      followed by [8] log prior_probs (DiscreteTransition.prior_probs, transitions.py:114-120; uniform = -log 8) */
  const float* tab_b;              /* [4][T] + [5]: same for bonds */
  const float* tab_score;          /* [T]: pos_score_coef (drift 'scale' option) */
  /* static inputs */
  const float* protein_pos;        /* [B,NP,3] centred (center_pos, decompdiff.py:20-32) */
  const float* protein_h;          /* [B,NP,128] protein embeddings + node indicator (dd_embed_protein) */
  const float* lig_aux;            /* [B,NL,2] */
  const float* atom_std;           /* [B,NL,3] prior_stds[ligand_decomp_batch] */
  const float* offset;             /* [B,3] protein centroid */
  const int32_t* decomp_index;     /* [B,NL] arm id or -1 (armsca drift); may be NULL */
  const float* full_protein_pos;   /* [B,NF,3] un-centred (clash drift); may be NULL */
  /* state, updated in place */
  float* lig_pos;                  /* [B,NL,3] centred x_t */
  int32_t* lig_v;                  /* [B,NL] */
  int32_t* lig_bond;               /* [B,NL*(NL-1)] */
  int32_t* step_counter;           /* [4] device ints, the run state: steps done so far in this run, t_start, seed lo,
                                      seed hi.  Written by dd_sampler_reset() from the t_start / seed fields of this
                                      struct; the kernels read the chain's start time and Philox key from HERE, so a
                                      captured step graph can be re-used for another chain of the same shape */
  /* drift (configs/sampling_drift.yml:31-37) */
  int32_t drift_armsca; float armsca_min_d, armsca_max_d; int32_t armsca_scale;
  int32_t drift_clash;  float clash_sigma, clash_gamma;    int32_t clash_scale;
  int32_t drift_norm_batch;        /* batch size the armsca loss is averaged over (guidance_funcs.py:78); 0 = B.
                                      Set when a larger (e.g. ragged) batch is run in several dense groups. */
  /* noise: injected (reference draw order, decompdiff.py:620,633,680) or Philox when NULL */
  const float* u_v;                /* [n_steps,B*NL,8]  uniforms for atom types   */
  const float* u_b;                /* [n_steps,B*Eb,5]  uniforms for bond types   */
  const float* eps;                /* [n_steps,B*NL,3]  normals for positions     */
  uint64_t seed;
  /* trajectories (may each be NULL): indexed by step */
  float* traj_pos;                 /* [n_steps,B*NL,3]  x_{t-1} + offset          */
  int32_t* traj_v;                 /* [n_steps,B*NL]                              */
  int32_t* traj_bond;              /* [n_steps,B*Eb]                              */
  float* traj_v0;                  /* [n_steps,B*NL,8]  log_softmax(v logits)     */
  float* traj_vt;                  /* [n_steps,B*NL,8]  posterior log-probs       */
  float* traj_bt;                  /* [n_steps,B*Eb,5]  bond posterior log-probs  */
  /* outputs of the last forward (always written) */
  float* pred_pos;                 /* [B,NL,3]  x0-hat (centred)                  */
  float* pred_v;                   /* [B,NL,8]  logits                            */
  float* pred_bond;                /* [B,Eb,5]  logits                            */
  /* scratch */
  float* workspace; size_t workspace_floats;
  /* heterogeneous batches ("padded/masked fixed-size pocket+ligand graphs"): samples with fewer atoms than NP / NL are
   * padded to the dense shape -- sample b's real protein atoms are rows 0 .. np_real[b]-1 of its protein block, its real
   * ligand atoms rows 0 .. nl_real[b]-1 of its ligand block (PyG collate of samples with different sizes:
   * utils/data.py:389-446, scripts/sample_diffusion_decomp.py:300-326).  Padding rows never enter a kNN list, a bond
   * or triplet segment, a softmax or a drift term; their own rows hold finite don't-care values.  NULL = dense. */
  const int32_t* np_real;          /* [B] or NULL */
  const int32_t* nl_real;          /* [B] or NULL */
  const int32_t* bl_prefix;        /* [B+1] prefix sums of nl_real*(nl_real-1) (compact enumeration of the real
                                      bond-layer segments); required when nl_real is given */
  /* Layer-0 tables (optional; all three NULL = off).  The first layer's projections and query rows are functions of the
   * embedded inputs alone: a ligand atom's rows depend on its (class, arm flag) -- 16 combinations -- a bond's on its
   * type (5) and its destination atom's combination, and the protein rows are the same in every step of a chain.  With
   * the tables set, a step gathers those rows instead of running the first layer's projection and query GEMMs
   * (models/common.py:85-105 MLP first Linear + the query MLPs of uni_transformer_edge.py:42-167).  Requires
   * lig_aux rows to be exactly (1,0) or (0,1) (utils/transforms.py arm / scaffold indicator) and a dense batch. */
  const float* l0_tables;          /* [DD_L0_TABLE_FLOATS], device; filled by dd_layer0_tables() once per weight set */
  float* l0_P;                     /* [B,N,640] layer-0 node projections; protein rows by dd_layer0_prepare() */
  float* l0_qn;                    /* [B,N,128] layer-0 node queries; protein rows by dd_layer0_prepare() */
  /* ABI 7: atom-class count of the checkpoint (0 = DD_NUM_V = 8; 13; 23): width of lig_v's range, of u_v, pred_v,
   * traj_v0 / traj_vt, of the v head's second Linear and (num_v + 2) of the ligand embedding's rows.  The layer-0 tables
   * exist for 8 classes only (l0_tables must be NULL otherwise). */
  int32_t num_v;
  /* ABI 8: arms_repul drift (utils/guidance_funcs.py:81-118; an EXTENSION of energy_drift_opt -- the reference defines the
   * energy but its sample_diffusion has no branch for it, models/decompdiff.py:643-675).  0 = off, 1 = mode 'min',
   * 2 = mode 'all'; evaluated at x_t like the other terms, scaled by pos_score_coef[t] when repul_scale is set. */
  int32_t drift_repul;
  float repul_max_d;
  int32_t repul_scale;
} dd_sampler;

/* Layout of l0_tables (floats): node projections [16][640], ligand projections [16][1280], bond projections [5][640],
 * node queries [16][128], node-with-bond queries [16][128], bond-layer queries [16 dst combinations][5 types][128].
 * Combination = 8 * (arm flag) + class.  A model with the narrow bond layer (see slot_off) keeps this layout: of a ligand row
 * the first 640 floats are used, the rest is unspecified and never gathered. */
#define DD_L0_TABLE_FLOATS (16 * 640 + 16 * 1280 + 5 * 640 + 16 * 128 + 16 * 128 + 80 * 128)
/* Build the tables: `mini` is a sampler with B = 1, NP = 0, NL = 16, K = 15 whose lig_v[i] = i % 8, lig_aux[i] = (i < 8 ?
 * (1,0) : (0,1)) and lig_bond[dst * 15 + s] = s % 5, with the model's weights and its own workspace; the SAME embedding,
 * projection and query kernels the forward uses run on it, so a gathered row equals the GEMM's row bit for bit. */
int dd_layer0_tables(const dd_sampler* mini, float* tables, void* stream);
/* Per chain (after protein_h is in place): the protein rows of s->l0_P and s->l0_qn. */
int dd_layer0_prepare(const dd_sampler* s, void* stream);

const char* dd_status_string(int status);
int dd_abi_version(void);
/* ABI 9: form of the attention MLPs in the packed arena that the kernels of this build expect.
 *   0 = canonical: the reference's values in the slot layout of decompdiff_amd/packing.py::pack_layer;
 *   1 = kernel form (packing.py::kernel_form_layer, exact algebra): every key / value MLP of the five attention sub-layers
 *       (models/encoders/uni_transformer_edge.py:42-74,125-167,188-210; MLP = models/common.py:85-105) has the channel mean of
 *       each additive first-Linear part removed (LayerNorm ignores it), sign(gamma) folded into those parts, |gamma| into the
 *       columns of the second Linear (W2k, W2v), beta / |gamma| in the LayerNorm slot's second row and the softmax scale
 *       1 / sqrt(8) inside W2k.  Same slots, shapes and offsets. */
int dd_weights_form(void);

/* (Re)start a chain: step_counter[0..3] = {0, s->t_start, s->seed}.  Must be enqueued on `stream` before the first
 * dd_sample_steps* / dd_graph_launch / dd_reverse_step of a chain. */
int dd_sampler_reset(const dd_sampler* s, void* stream);

/* Floats of workspace needed by dd_forward/dd_sample_steps for these shapes. */
size_t dd_workspace_floats(int B, int NP, int NL, int K);

/* torch_geometric.nn.knn_graph -> torch_cluster.knn (call site uni_transformer_edge.py:353):
 * per-sample K nearest other atoms, ascending (d2, index); d2 = (dx*dx+dy*dy)+dz*dz in fp32. */
int dd_knn(const float* x /*[B,N,3]*/, int B, int N, int K, int32_t* nbr /*[B,N,K]*/, void* stream);
/* The same for a padded heterogeneous batch in the layout of dd_sampler.np_real / nl_real (NP + NL rows per sample, the real atoms
 * first in each block; np_real may be NULL = all NP rows real): padding atoms are neither centres nor candidates; the list of a
 * padding centre is zeros.  Every sample needs at least K + 1 real atoms.  (Round 5: the padded training network.) */
int dd_knn_masked(const float* x /*[B,NP+NL,3]*/, int B, int NP, int NL, int K, const int32_t* np_real, const int32_t* nl_real,
                  int32_t* nbr /*[B,NP+NL,K]*/, void* stream);
/* torch_geometric.nn.knn_graph(x, k, batch, loop) on a flat PyG batch of DIFFERENT samples (the reference's loader collates
 * different complexes, utils/data.py:389-446): sample b owns rows ptr[b] .. ptr[b+1]-1 of x (ptr[0] = 0, non-decreasing,
 * ptr[B] = n; any count per sample, 0, 1 and more than DD_N_MAX included).  Its centres get k_b = min(K, n_b - 1) neighbours
 * (loop = 1: the centre is a candidate itself, k_b = min(K, n_b)), in the order of dd_knn -- a dense batch gives dd_knn's lists.
 * out_off[b] = sum over b' < b of n_b' * k_b' and E = out_off[B] (host prefix sums; device pointers like ptr).  The kernel writes
 * GLOBAL row ids as int64 into the compact edge_index [2,E]: row 0 the neighbour, row 1 the centre; edges grouped by centre in
 * ascending row order.  One wave per centre streams the sample's rows in chunks of at most DD_N_MAX and carries the k_b best keys
 * between chunks: exact for every size.  n_max = the largest n_b (picks the chunk size only; any value gives the same result).
 * Rows outside [0,n) and edges outside [0,E) are never touched, whatever ptr / out_off hold.  K <= DD_KNN_MAX.
 * (New entry point, ABI unchanged.) */
int dd_knn_csr(const float* x /*[n,3]*/, const int32_t* ptr /*[B+1]*/, int B, int n, int n_max, int K, int loop,
               const int64_t* out_off /*[B+1]*/, int64_t E, int64_t* edge_index /*[2,E]*/, void* stream);

/* e_w = sigmoid(MLP(GaussianSmearing(dist)))  (uni_transformer_edge.py:422-427). */
int dd_edge_weights(const float* x, const int32_t* nbr, int B, int N, int K, const float* W1T /*[20,128]*/,
                    const float* b1, const float* ln /*[2,128]*/, const float* w2 /*[128]*/, const float* b2 /*[1]*/,
                    float* ew /*[B,N,K]*/, void* stream);

/* nn.Linear / MLP first-layer projections (ATen addmm call sites in models/common.py:85-105):
 * Y[r, 0:ncols] (+)= op(X[r, 0:128]) * W[ncols,128]^T + bias, fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * Row r of X lives at X + (r / x_rows_per_b) * x_stride_b + (r % x_rows_per_b) * ldx (floats);
 * same for Y.  ln != NULL applies LayerNorm(gamma,beta)+ReLU to each X row first (the MLP's
 * hidden activation); accumulate != 0 adds into Y. */
int dd_gemm128(const float* X, int x_rows_per_b, long x_stride_b, int ldx, int rows, const float* W,
               const float* bias, const float* ln, float* Y, int y_rows_per_b, long y_stride_b, int ldy,
               int ncols, int accumulate, void* stream);

/* nn.Linear backward of the training step (scripts/train_diffusion_decomp.py; the ATen mm calls autograd makes behind
 * models/common.py:85-105), weight gradient:  out[M,128] (+)= A[rows,M]^T * X[rows,128]  (A = dY, M <= 128 output channels,
 * row r of A at A + r*lda, of X at X + r*ldx, of out at out + o*ldo).  The input gradient dX = dY * W is dd_gemm128 with the
 * transposed weight.  fp32 MFMA, slabs of rows reduced in a fixed order (bitwise reproducible, no atomics);
 * scratch: dd_gemm128_tn_scratch_floats(rows, M) floats. */
size_t dd_gemm128_tn_scratch_floats(long rows, int M);
int dd_gemm128_tn(const float* A, int lda, int M, const float* X, int ldx, long rows, float* scratch, float* out, int ldo,
                  int accumulate, void* stream);
/* ... with the bias gradient of the same Linear: bias_out[M] = column sums of A (dY^T 1; autograd's dy.sum(0)), formed from the
 * rows the kernel stages anyway, slabs added in the same fixed order.  Same scratch size.  (Added in round 5; ABI unchanged:
 * a new entry point, no struct layout touched.) */
int dd_gemm128_tn_bias(const float* A, int lda, int M, const float* X, int ldx, long rows, float* scratch, float* out, int ldo,
                       int accumulate, float* bias_out, void* stream);

/* LayerNorm(128) + ReLU of the reference's MLPs (models/common.py:85-105) for the training step, one kernel each way:
 *   forward : y[r] = relu(LN(x[r]) * gamma + beta) (eps 1e-5), stats[r] = (mean, 1/std) kept for the backward;
 *   backward: dx from dy (the ReLU mask is recomputed from x), dgamma[128] / dbeta[128] summed over the rows in a fixed order
 *             (no atomics); scratch: dd_ln_relu_scratch_floats(rows) floats.
 * Rows are contiguous [rows,128] fp32; x / y / dy / dx / gamma / beta 16-byte aligned (read as float4), stats 8-byte aligned
 * (checked: DD_ERR_BAD_ARG otherwise); rows == 0 is DD_OK both ways.  (Round 5; new entry points, ABI unchanged.) */
size_t dd_ln_relu_scratch_floats(long rows);
int dd_ln_relu_forward(const float* x, const float* gamma, const float* beta, float* y, float* stats, long rows, void* stream);
int dd_ln_relu_backward(const float* x, const float* stats, const float* gamma, const float* beta, const float* dy, float* dx,
                        float* scratch, float* dgamma, float* dbeta, long rows, void* stream);

/* Op-level message passing: the torch_scatter pairs of the reference's attention layers as stand-alone ops
 *     alpha = scatter_softmax((q[dst] * k / sqrt(8)).sum(-1), dst, dim=0);  out = scatter_sum(alpha[..., None] * v, dst, dim=0)
 * (uni_transformer_edge.py:63-68 NodeUpdateLayer, :158-164 BondUpdateLayer, :205-211 PosUpdateLayer).  16 heads x 8
 * channels.  Edges grouped by destination: seg_ptr[s] .. seg_ptr[s+1] are the edges of destination s (knn_graph's,
 * the dst-major bond list's and the SparseTensor triplets' order).  v is multiplied by e_w[edge] when e_w != NULL
 * (:55-56).  q is [n_seg,128], or per edge [E,128] with q_per_edge != 0 (rows of a segment are then identical and
 * the first is read).  Destinations without edges get zeros.  The sampling loop does not call these (its fused
 * kernels never materialise q / k / v); they serve hosts that keep the reference's Python layers. */
int dd_attn_aggregate_node(const float* q, int q_per_edge, const float* k /*[E,128]*/, const float* v /*[E,128]*/,
                           const float* e_w /*[E] or NULL*/, const int32_t* seg_ptr /*[n_seg+1]*/, int n_seg,
                           float* out /*[n_seg,128]*/, void* stream);
/* BondUpdateLayer form: q per triplet, no e_w. */
int dd_attn_aggregate_triplet(const float* q /*[E3,128]*/, const float* k, const float* v, const int32_t* seg_ptr, int n_seg,
                              float* out /*[n_seg,128]*/, void* stream);
/* PosUpdateLayer form: v16 [E,16] per head, rel_x [E,3]; out[s] = mean_heads(sum_e alpha * v16 * e_w * rel_x) [n_seg,3]. */
int dd_attn_aggregate_pos(const float* q /*[n_seg,128]*/, const float* k, const float* v16, const float* e_w, const float* rel_x,
                          const int32_t* seg_ptr, int n_seg, float* out /*[n_seg,3]*/, void* stream);
/* Backward of the pair above (training hosts): gradients of q, k, v (v16), e_w and rel_x from d_out, the gradient of the
 * output.  The scores are recomputed (nothing is saved by the forward); the node form also reads `out`, the forward's result.
 * dq has q's shape ([n_seg,128], or [E,128] with q_per_edge != 0: dq[e] = scale * ds[e] * k[e] per edge).  d_ew is NULL
 * exactly when e_w is NULL (DD_ERR_BAD_ARG otherwise).  No atomics: every element of every output is written once, except
 * that an empty segment writes only its zero dq row (q per segment) -- bitwise reproducible, and the buffers need no
 * initialisation.  The triplet form is the node form with q_per_edge = 1 and e_w = NULL.  (New entry points, ABI unchanged.) */
int dd_attn_aggregate_node_bwd(const float* q, int q_per_edge, const float* k, const float* v, const float* e_w /*NULL ok*/,
                               const int32_t* seg_ptr, int n_seg, const float* out /*[n_seg,128]*/, const float* d_out /*[n_seg,128]*/,
                               float* dq, float* dk /*[E,128]*/, float* dv /*[E,128]*/, float* d_ew /*[E]; NULL iff e_w NULL*/,
                               void* stream);
int dd_attn_aggregate_pos_bwd(const float* q /*[n_seg,128]*/, const float* k, const float* v16, const float* e_w /*NULL ok*/,
                              const float* rel_x, const int32_t* seg_ptr, int n_seg, const float* d_out /*[n_seg,3]*/,
                              float* dq /*[n_seg,128]*/, float* dk /*[E,128]*/, float* dv16 /*[E,16]*/,
                              float* d_ew /*[E]; NULL iff e_w NULL*/, float* d_rel /*[E,3]*/, void* stream);
/* Member masks (padded batches): the four entry points above with member_mask [E] after seg_ptr / n_seg; a non-zero byte
 * means the member is real.  A masked member does not exist: the softmax of a segment runs over its real members only, in
 * member order, with bit for bit the results of the same call on arrays compacted to the real members; a segment without a
 * real member (empty or all masked) gives a zero output row.  The k, v (v16), e_w and rel_x rows of a masked member -- with
 * q_per_edge != 0 its q row too: q is read from the segment's first real member -- reach no result, whatever they hold (NaN
 * and Inf included).  Backward: a masked member gets exactly 0 in dk, dv, d_ew, d_rel (and in its dq row with
 * q_per_edge != 0); a segment without a real member writes those zeros and its zero dq row (q per segment).  Every element
 * is still written exactly once, without atomics.  member_mask == NULL: all members are real -- the unmasked entry point's
 * launch and results.  Argument checks as for the siblings.  (New entry points, ABI unchanged.) */
int dd_attn_aggregate_node_masked(const float* q, int q_per_edge, const float* k, const float* v, const float* e_w /*NULL ok*/,
                                  const int32_t* seg_ptr, int n_seg, const uint8_t* member_mask /*[E] or NULL*/,
                                  float* out /*[n_seg,128]*/, void* stream);
int dd_attn_aggregate_pos_masked(const float* q, const float* k, const float* v16, const float* e_w /*NULL ok*/, const float* rel_x,
                                 const int32_t* seg_ptr, int n_seg, const uint8_t* member_mask /*[E] or NULL*/,
                                 float* out /*[n_seg,3]*/, void* stream);
int dd_attn_aggregate_node_bwd_masked(const float* q, int q_per_edge, const float* k, const float* v, const float* e_w /*NULL ok*/,
                                      const int32_t* seg_ptr, int n_seg, const uint8_t* member_mask /*[E] or NULL*/,
                                      const float* out, const float* d_out, float* dq, float* dk, float* dv, float* d_ew,
                                      void* stream);
int dd_attn_aggregate_pos_bwd_masked(const float* q, const float* k, const float* v16, const float* e_w /*NULL ok*/,
                                     const float* rel_x, const int32_t* seg_ptr, int n_seg,
                                     const uint8_t* member_mask /*[E] or NULL*/, const float* d_out, float* dq, float* dk,
                                     float* dv16, float* d_ew, float* d_rel, void* stream);

/* Stand-alone torch_scatter drop-ins over dim 0 of a [E,F] fp32 tensor whose rows are grouped by destination (CSR
 * segments seg_ptr [n_seg+1]); reference call sites: scatter_softmax / scatter_sum uni_transformer_edge.py:64,68,160,164,
 * 205,209, scatter_mean decompdiff.py:25 (center_pos), scatter_min guidance_funcs.py:52.
 * dd_segment_reduce: op 0 sum, 1 mean, 2 min, 3 max -> out [n_seg,F]; empty segments give 0 (torch_scatter's fill);
 * min / max also write the row index of the extremum to arg_out [n_seg,F] (may be NULL; E for an empty segment, the
 * smallest index on ties).  dd_segment_softmax: out[e,f] = exp(src[e,f] - max_seg) / sum_seg exp(...), [E,F]. */
int dd_segment_reduce(const float* src, const int32_t* seg_ptr, int n_seg, int F, int op, long E, float* out,
                      int64_t* arg_out, void* stream);
int dd_segment_softmax(const float* src, const int32_t* seg_ptr, int n_seg, int F, float* out, void* stream);

/* torch_sparse.SparseTensor at its one call site, BondUpdateLayer.triplets (uni_transformer_edge.py:103-123): a CSR built on the
 * device and rows selected from it, with an optional key to leave out per selected row.
 *   CSR: entry e of a COO list sits in row node[e] with key key[e] (int64, E entries; any order; rows without entries are
 *        normal).  Every row's run is ordered by (key, e): the stable (row, col) order of the SparseTensor.
 *   Selection: for r < R, in order, the members of row sel[r] in run order, except those whose key equals skip[r] (skip NULL:
 *        none left out).  Per surviving member t: out_row[t] = r, out_key[t] = its key, out_entry[t] = its entry id e,
 *        out_sel[t] = sel[r], out_skip[t] = skip[r]; each out_* may be NULL (not written).
 * The triplets (k->j->i) of the directed graph row[e] -> col[e] (j -> i) are the selection node = col, key = row, sel = row,
 * skip = col, R = E over n_rows = n_cols = num_nodes:  idx_ji = out_row, idx_k = out_key, idx_kj = out_entry, idx_j = out_sel,
 * idx_i = out_skip -- for every edge in edge order the edges into its source, k ascending (equal (k, j) in edge order), k == i
 * dropped; a self loop is an edge like any other.  `t[index]` of the SparseTensor is the selection with skip = NULL.
 * Two phases, because the size of the result depends on the data:
 *   dd_csr_select_scratch_bytes: bytes of scratch for these sizes (0: refused, see below);
 *   dd_csr_select_count: builds the CSR and the offsets in `scratch` (8-byte aligned, caller-owned) and leaves two int64 at its
 *        start: scratch[0] = total, the number of surviving members, scratch[1] = bad, the number of entries with node[e]
 *        outside [0, n_rows) or key[e] outside [0, n_cols) plus the number of sel[r] outside [0, n_rows).  Such entries belong
 *        to no row and such a selection is empty: nothing outside the caller's buffers is read or written, whatever the ids hold;
 *   dd_csr_select_fill: after the caller has read `total` and allocated the lists, with the same sel / skip / sizes / scratch.
 *        At most `total` and at most the counted number of elements of each list are written.
 * Internally int32: E, n_rows, n_cols, R or a total at or above 2^31 give DD_ERR_UNSUPPORTED_SHAPE.  Runs may have any length
 * (no per-row buffer); ordering a run costs its length squared.  Integer atomics only place entries before the ordering, so
 * the results are bit-identical from run to run.  (New entry points, ABI unchanged.) */
size_t dd_csr_select_scratch_bytes(int64_t E, int64_t n_rows, int64_t n_cols, int64_t R);
int dd_csr_select_count(const int64_t* node /*[E]*/, const int64_t* key /*[E]*/, int64_t E, int64_t n_rows, int64_t n_cols,
                        const int64_t* sel /*[R]*/, const int64_t* skip /*[R] or NULL*/, int64_t R, void* scratch,
                        size_t scratch_bytes, void* stream);
int dd_csr_select_fill(const int64_t* sel, const int64_t* skip, int64_t E, int64_t n_rows, int64_t n_cols, int64_t R,
                       const void* scratch, int64_t total, int64_t* out_row, int64_t* out_key, int64_t* out_entry,
                       int64_t* out_sel, int64_t* out_skip, void* stream);

/* Embeddings (decompdiff.py:219-256, 296-297). protein_h is step-invariant. */
int dd_embed_protein(const float* protein_v /*[B*NP,29]*/, int rows, const float* W /*[128,29]*/, const float* b,
                     float* protein_h /*[rows,128]*/, void* stream);

/* Whole score network once: DecompScorePosNet3D.forward for the shipped config
 * (decompdiff.py:213-351 -> uni_transformer_edge.py:394-443).  Reads s->lig_pos/lig_v/lig_bond,
 * writes s->pred_pos/pred_v/pred_bond. */
int dd_forward(const dd_sampler* s, void* stream);

/* One reverse transition from network outputs the host computed itself (decompdiff.py:601-689 without the forward):
 * log_softmax + q_v_posterior + log_sample_categorical for atoms and bonds (logits_v [B*NL,8], logits_b [B*Eb,5]),
 * posterior mean from x0 [B*NL,3] (centred; the network's coordinate output -- for a noise-mode model s->tab_pos holds
 * the folded rows, see dd_sampler.tab_pos), drift, noise; updates s->lig_pos / lig_v / lig_bond, writes the
 * trajectories at the current step index and advances s->step_counter -- exactly what a step of dd_sample_steps does
 * after its forward (bit-identical when fed dd_forward's pred_*). */
int dd_reverse_step(const dd_sampler* s, const float* logits_v, const float* logits_b, const float* x0, void* stream);

/* n_steps iterations of the reverse loop (decompdiff.py:575-689): forward, categorical
 * posteriors + Gumbel-argmax, Gaussian posterior mean, optional drift, noise, trajectories. */
int dd_sample_steps(const dd_sampler* s, int n_steps, void* stream);

/* Same loop with one step captured into a hipGraph and replayed n_steps times. */
int dd_sample_steps_graph(const dd_sampler* s, int n_steps, void* stream);

/* The same, split so that a host can interleave its own work (e.g. draining trajectory chunks to the host on a copy
 * stream) with the replays: create captures `steps_per_graph` (>= 1) consecutive steps of chain `s` on `stream` into one
 * executable graph; launch replays it n_graphs times on `stream` without waiting; destroy waits for nothing — the
 * caller synchronises the stream first.  The dd_sampler and every buffer it points to must stay alive and unchanged
 * until the graph is destroyed. */
int dd_graph_create(const dd_sampler* s, int steps_per_graph, void* stream, void** graph_out /*HOST*/);
int dd_graph_launch(void* graph, int n_graphs, void* stream);
int dd_graph_destroy(void* graph);

/* n independent chains advanced together: chain i's step graph is captured on streams[i] (HOST array of n distinct,
 * non-default streams) and the n graphs are replayed round-robin, so chains with different sizes (the sub-batches of
 * a heterogeneous PyG batch: sample_diffusion_decomp.py:300-326 collates samples with different ligand sizes when
 * num_atoms_mode is 'prior' / 'old' / 'stat') share the GPU instead of running back to back.  Every chain needs its
 * own workspace and state buffers.  Waits for all streams before returning. */
int dd_sample_steps_graph_multi(const dd_sampler* const* s /*HOST [n]*/, int n, int n_steps,
                                void* const* streams /*HOST [n]*/);

/* Bond head of the model (decompdiff.py:199-211, 323-341).  The entry points without the _ex suffix run the 'lin' head
 * (bond_inference on the last layer's h_bond, slots DD_G_BH_W1 / DD_G_BH_b1); they equal the _ex variants with bh = NULL.
 * 'pre_att' reads the final coordinates and atom features: for ligand bond e = (src, dst),
 *   hidden[e] = W_r^T r(d) + P[dst] + P[src] + b1,  d = |x_dst - x_src| of the network's output coordinates,
 *   r_k(d) = exp(coeff * (d - offset[k])^2) (k < 20),  P = W_p h of the final h (ligand rows),
 * where W_p = W1[:, 20:148] / 2 and W_r = W1[:, 0:20]^T of the reference's bond_inference.0 (W1 [128, 148], bias b1); the
 * second Linear stays in the slots DD_G_BH_W2 / DD_G_BH_b2.  All pointers are DEVICE pointers and must stay valid while a
 * graph captured with the descriptor is alive. */
#define DD_BOND_HEAD_LIN 0
#define DD_BOND_HEAD_PRE_ATT 1
typedef struct dd_bond_head {
  int32_t kind;            /* DD_BOND_HEAD_LIN or DD_BOND_HEAD_PRE_ATT */
  int32_t num_r;           /* Gaussians of the distance expansion: 20 */
  const float* W_p;        /* [128, 128] (out, in): the feature half of W1, halved */
  const float* W_r;        /* [20, 128]: the distance columns of W1, transposed */
  const float* b1;         /* [128] */
  const float* offset;     /* [20] centres of the distance expansion */
  float coeff;             /* its exponent factor, -0.5 / (offset[1] - offset[0])^2 */
  int32_t reserved;
} dd_bond_head;

/* dd_forward / dd_sample_steps / dd_sample_steps_graph / dd_graph_create / dd_sample_steps_graph_multi with a bond head
 * (NULL or kind DD_BOND_HEAD_LIN: exactly the functions above).  bh of the multi variant: HOST array of n descriptors
 * (entries may be NULL), or NULL for all lin. */
int dd_forward_ex(const dd_sampler* s, const dd_bond_head* bh /*HOST*/, void* stream);
int dd_sample_steps_ex(const dd_sampler* s, const dd_bond_head* bh /*HOST*/, int n_steps, void* stream);
int dd_sample_steps_graph_ex(const dd_sampler* s, const dd_bond_head* bh /*HOST*/, int n_steps, void* stream);
int dd_graph_create_ex(const dd_sampler* s, const dd_bond_head* bh /*HOST*/, int steps_per_graph, void* stream,
                       void** graph_out /*HOST*/);
int dd_sample_steps_graph_multi_ex(const dd_sampler* const* s /*HOST [n]*/, const dd_bond_head* const* bh /*HOST [n]*/, int n,
                                   int n_steps, void* const* streams /*HOST [n]*/);

/* Node output MLPs (x2h_out_fc: True; uni_transformer_edge.py:39-40, 70-71).  Each NodeUpdateLayer of a layer then ends in
 * node_output = MLP(256 -> 128, LayerNorm, ReLU, 128 -> 128) on cat([aggregate, h]), and the layer's node update is
 *   z_e = relu(LN_e(W1_e [A_e ; h] + b1_e)),  z_b = relu(LN_b(W1_b [A_b ; h] + b1_b))   (A_b = 0 on protein rows),
 *   h_new = h + W2_e' z_e + W2_b' z_b + c0,   W2_m' = W_lin W2_m,  c0 = W_lin (b2_e + b2_b) + b_lin   (composed on the host).
 * A layer's weights are one DEVICE block of DD_NO_BLOCK_FLOATS floats (16-byte aligned) at the offsets below; W1_* are
 * [128, 256] (out, in) as in the checkpoint, W2_*' [128, 128] (out, in), ln_* [2, 128] gamma ; beta.  The entry points without a
 * dd_node_out run the model without these MLPs (h_new = h + W_lin (A_e + A_b) + b_lin from the slots DD_W_lin / DD_b_lin). */
#define DD_NO_W1E 0
#define DD_NO_W1B 32768
#define DD_NO_W2E 65536
#define DD_NO_W2B 81920
#define DD_NO_B1E 98304
#define DD_NO_B1B 98432
#define DD_NO_LNE 98560
#define DD_NO_LNB 98816
#define DD_NO_C0 99072
#define DD_NO_BLOCK_FLOATS 99200
typedef struct dd_node_out {
  int32_t num_layers;      /* = dd_sampler.num_layers */
  int32_t reserved;
  const float* layer[64];  /* DEVICE block of each layer; must stay valid while a graph captured with the descriptor is alive */
} dd_node_out;

/* The kernel alone: h_out[B (NP + NL), 128] = the node update above from A_e [B (NP + NL), 128], A_b [B NL, 128] (ligand rows
 * only), h [B (NP + NL), 128] and one layer block `weights`; h_out may be h.  np_real / nl_real (padded batches, may be NULL):
 * padding rows are computed like real ones, as the lin_node GEMM does -- finite inputs give finite rows nobody reads. */
int dd_node_out_fc(const float* A_e, const float* A_b, const float* h, int B, int NP, int NL, const float* weights,
                   const int32_t* np_real, const int32_t* nl_real, float* h_out, void* stream);

/* The _ex entry points with both descriptors (no NULL: exactly the _ex functions, which call these).  no of the multi variant:
 * HOST array of n descriptors (entries may be NULL), or NULL. */
int dd_forward_ex2(const dd_sampler* s, const dd_bond_head* bh /*HOST*/, const dd_node_out* no /*HOST*/, void* stream);
int dd_sample_steps_ex2(const dd_sampler* s, const dd_bond_head* bh /*HOST*/, const dd_node_out* no /*HOST*/, int n_steps, void* stream);
int dd_sample_steps_graph_ex2(const dd_sampler* s, const dd_bond_head* bh /*HOST*/, const dd_node_out* no /*HOST*/, int n_steps,
                              void* stream);
int dd_graph_create_ex2(const dd_sampler* s, const dd_bond_head* bh /*HOST*/, const dd_node_out* no /*HOST*/, int steps_per_graph,
                        void* stream, void** graph_out /*HOST*/);
int dd_sample_steps_graph_multi_ex2(const dd_sampler* const* s /*HOST [n]*/, const dd_bond_head* const* bh /*HOST [n]*/,
                                    const dd_node_out* const* no /*HOST [n]*/, int n, int n_steps, void* const* streams /*HOST [n]*/);

/* Model options: everything a model is beyond its dd_sampler, in ONE struct that can grow -- the end of the _ex / _ex2 suffix
 * chain.  `size` is the caller's sizeof(dd_model_opts): the library reads no field beyond it and takes the default for the
 * rest (NULL descriptors, one block), so a program built against this version keeps running on a library that knows more
 * fields.  opts == NULL: all defaults.
 *   num_blocks: blocks of the refine net (uni_transformer_edge.py:402-437).  The network runs num_blocks * num_layers steps;
 *   step l uses the weight slots of layer l % num_layers (the blocks share their weights), and in front of every block but
 *   the first the kNN graph and the edge weights are rebuilt from the coordinates the previous block left (one launch; the
 *   same neighbour order and e_w arithmetic as the first block's).  The layer-0 tables serve the very first step only.
 *   num_blocks >= 1 and num_blocks * num_layers <= 64 (DD_ERR_BAD_ARG / DD_ERR_UNSUPPORTED_SHAPE otherwise); node_out keeps
 *   describing ONE block (node_out->num_layers == dd_sampler.num_layers).  dd_workspace_floats sizes the workspace for any
 *   block count.  Every entry point without a dd_model_opts means num_blocks = 1.  (New entry points, ABI unchanged.) */
typedef struct dd_model_opts {
  int32_t size;                  /* sizeof(dd_model_opts) of the caller */
  const dd_bond_head* bond_head; /* HOST, may be NULL (the lin head) */
  const dd_node_out* node_out;   /* HOST, may be NULL (no x2h_out_fc) */
  int32_t num_blocks;            /* >= 1 */
} dd_model_opts;
/* The _ex2 entry points with the options struct (the _ex2 functions call these with num_blocks = 1).  opts of the multi
 * variant: HOST array of n pointers (entries may be NULL), or NULL. */
int dd_forward_opts(const dd_sampler* s, const dd_model_opts* opts /*HOST*/, void* stream);
int dd_sample_steps_opts(const dd_sampler* s, const dd_model_opts* opts /*HOST*/, int n_steps, void* stream);
int dd_sample_steps_graph_opts(const dd_sampler* s, const dd_model_opts* opts /*HOST*/, int n_steps, void* stream);
int dd_graph_create_opts(const dd_sampler* s, const dd_model_opts* opts /*HOST*/, int steps_per_graph, void* stream,
                         void** graph_out /*HOST*/);
int dd_sample_steps_graph_multi_opts(const dd_sampler* const* s /*HOST [n]*/, const dd_model_opts* const* opts /*HOST [n]*/, int n,
                                     int n_steps, void* const* streams /*HOST [n]*/);

/* Per-sample noise keys: a sample's production noise independent of the batch it sits in.  The two _opts entry points above
 * with one more DEVICE pointer, sample_keys [B] uint64.  Sample b then receives exactly the draws that a chain of that sample
 * alone (B = 1) with dd_sampler.seed = sample_keys[b] receives, at any position of a dense or padded batch of any B:
 *   atom types   stream 1, Philox key sample_keys[b], counter row i (the atom's index in its sample)
 *   bond types   stream 2, key sample_keys[b], counter row dst * (n - 1) + sp with sp = src - (src > dst) and n the sample's
 *                real ligand size (nl_real[b] in a padded batch, NL otherwise): the row of the sample's OWN dst-major bond
 *                list, not of the padded one.  Rows of padding bonds draw at their padded row (nobody reads them).
 *   coordinates  stream 7, key sample_keys[b], index 3 * i + c
 * Philox4x32-10 with counter (row, row >> 32, t, stream | class block << 8) as for dd_sampler.seed; t stays the diffusion time
 * index, so a chain resumed with another t_start and the same keys continues the unsplit chain's noise.  dd_sampler.seed is
 * not read.  The keys are read from device memory at every launch (never baked into a graph): a graph from
 * dd_graph_create_keyed serves every later chain of its shape once other keys are copied into the same buffer, and
 * dd_graph_launch / dd_graph_destroy take it like any other.
 *   sample_keys == NULL: exactly dd_sample_steps_opts / dd_graph_create_opts.
 *   sample_keys together with injected noise (any of s->u_v / u_b / eps): DD_ERR_BAD_ARG.
 * dd_reverse_step and the dd_sample_steps_graph* / _multi* entry points stay unkeyed.  (New entry points, ABI unchanged.) */
int dd_sample_steps_keyed(const dd_sampler* s, const dd_model_opts* opts /*HOST*/, const uint64_t* sample_keys /*DEVICE [B]*/,
                          int n_steps, void* stream);
int dd_graph_create_keyed(const dd_sampler* s, const dd_model_opts* opts /*HOST*/, const uint64_t* sample_keys /*DEVICE [B]*/,
                          int steps_per_graph, void* stream, void** graph_out /*HOST*/);

/* Fixed atoms (EXTENSION; generalises the reference's ligand_atom_mask hook, decompdiff.py:597,621-622,682-683, which its own
 * loop cannot run): some ligand atoms are KNOWN and are held, or re-noised, at every reverse step while the rest is sampled.
 * The network and the drift terms always see the whole ligand; pred_*, traj_v0 / traj_vt / traj_bt stay what the network and
 * the posterior say for every row, and a free row steps exactly as without `fixed`, with the very same draws.
 *   mask [B*NL] uint8: != 0 -- the atom is held.  A bond row is held iff BOTH its endpoints are: row r of a sample has
 *     dst = r / (NL - 1), sp = r % (NL - 1), src = sp + (sp >= dst).  Padding atoms of a padded batch must carry 0.
 *   v0 [B*NL] int32, b0 [B*NL*(NL-1)] int32, x0c [B*NL,3] float: the known clean classes / centred coordinates (x - offset of
 *     the sample); read at held rows only.
 *   DD_FIXED_HOLD: every step writes the known values into the state (and the trajectories) of the held rows.
 *   DD_FIXED_REPLACE (RePaint): the step at time t leaves the held rows at a fresh sample of the forward process at level
 *     t - 1 (decompdiff.py:436-455, transitions.py:146-150), drawn with the row's OWN draws of that step -- those a free row
 *     spends on its transition: injected u_v / u_b / eps rows, or Philox (key, row, t, stream) as addressed above --
 *       x = A[t-1] * (x0c - cc) + (S[t-1] * e) * atom_std + cc       cc [B*NL,3]: centred prior centre of the atom's arm,
 *                                                                    tab [2][T]: A = sqrt(alphas_cumprod), S = sqrt(1 - A^2)
 *       class = argmax_c gumbel(u_c) + log_add_exp(log_onehot(v0)_c + log_cumprod[t-1], log_1m_cumprod[t-1] + log_prior_c)
 *     and the step at t = 0 leaves x0c / v0 / b0 themselves.  "Level l of a held row is drawn at time l + 1", always.
 *   dd_fixed_init: prepares the state in front of the first step -- HOLD: the known values; REPLACE: level t_start with the
 *     same formulas and streams at Philox time t_start + 1 (after dd_sampler_reset; no injected noise: DD_ERR_BAD_ARG), so a
 *     chain split with another t_start continues the unsplit one.  A host that supplies level t_start itself skips the call.
 * All pointers are DEVICE pointers read at every launch: a graph from dd_graph_create_fixed serves every chain of its shape
 * and mode, whatever the mask and the known values.  `size` is the caller's sizeof(dd_fixed), as in dd_model_opts.
 *   fixed == NULL: exactly the _keyed entry point (dd_fixed_init: DD_ERR_BAD_ARG).  A NULL mask / v0 / b0 / x0c, an unknown mode,
 *   REPLACE without cc / tab: DD_ERR_BAD_ARG before any launch.  dd_reverse_step stays unfixed.  (New entry points, ABI unchanged.) */
enum { DD_FIXED_HOLD = 1, DD_FIXED_REPLACE = 2 };
typedef struct dd_fixed {
  int32_t size;                  /* sizeof(dd_fixed) of the caller */
  int32_t mode;                  /* DD_FIXED_HOLD / DD_FIXED_REPLACE */
  const uint8_t* mask;           /* DEVICE [B*NL] */
  const int32_t* v0;             /* DEVICE [B*NL] */
  const int32_t* b0;             /* DEVICE [B*NL*(NL-1)] */
  const float* x0c;              /* DEVICE [B*NL,3] */
  const float* cc;               /* DEVICE [B*NL,3], REPLACE only */
  const float* tab;              /* DEVICE [2][T], REPLACE only */
} dd_fixed;
int dd_sample_steps_fixed(const dd_sampler* s, const dd_model_opts* opts /*HOST*/, const uint64_t* sample_keys /*DEVICE [B] or NULL*/,
                          const dd_fixed* fixed /*HOST*/, int n_steps, void* stream);
int dd_graph_create_fixed(const dd_sampler* s, const dd_model_opts* opts /*HOST*/, const uint64_t* sample_keys /*DEVICE [B] or NULL*/,
                          const dd_fixed* fixed /*HOST*/, int steps_per_graph, void* stream, void** graph_out /*HOST*/);
int dd_fixed_init(const dd_sampler* s, const uint64_t* sample_keys /*DEVICE [B] or NULL*/, const dd_fixed* fixed /*HOST*/, void* stream);

/* Resampling (EXTENSION; the other half of RePaint beside DD_FIXED_REPLACE): after some reverse steps the whole ligand is diffused
 * FORWARD again by jump_length levels and denoised once more, so that the free atoms get several passes in which to agree with
 * the held ones.  The host owns the schedule (decompdiff_amd.resample_schedule: runs of reverse steps with a jump between them);
 * the library supplies the jump, fresh draws for a revisited time, and step entry points that honour them.
 *   Levels: a state is at level l in {-1, 0, .., T-1}; the reverse step at time t takes level t to t - 1; level -1 is what the
 *     step at t = 0 leaves (the clean sample), with alphas_cumprod[-1] = 1 for all three schedules.  The chain's current level is
 *     l = t_start - steps done of the run state (step_counter).
 *   dd_resample_jump: the forward transition q(x_m | x_l), m = l + jump_length, in ONE launch over coordinates, atom rows and
 *     bond rows, coefficients from tab [6][T] at m (rows A, S, lr_v, l1mr_v, lr_b, l1mr_b; composed in float64 by the host and
 *     rounded once; entries m < jump_length - 1 are never read):
 *       x' = A * (x - cc) + (S * e) * atom_std + cc        A = sqrt(abar[m] / abar[l]), S = sqrt(1 - abar[m] / abar[l]), cc as in
 *                                                          dd_fixed (REQUIRED here in both modes), every operation rounded on
 *                                                          its own; the jump_length-fold composition of decompdiff.py:436-447
 *       class' = argmax_c gumbel(u_c) + log_add_exp(log_onehot(class)_c + lr, l1mr + log_prior_c)
 *                                                          lr = log_cumprod[m] - log_cumprod[l], l1mr = log(1 - exp(lr)):
 *                                                          transitions.py:123-133 composed (exact for any prior)
 *     DD_FIXED_REPLACE: every row moves (a held row at level m is then a valid forward sample of its clean value).
 *     DD_FIXED_HOLD: held atoms, and bonds with both endpoints held, keep their bits; every other row moves.  Drift terms play no
 *     part, and a jumped state is written to no trajectory: trajectory position p is the state after the p-th reverse step of the
 *     call (steps done keeps counting through jumps).  A one-thread launch behind the jump rebases the run state
 *     (t_start += jump_length, so the next step runs at time m) and adds 1 to *epoch.  m must be < T (the host's schedule sees to it).
 *   Fresh draws: *epoch = jumps done so far in the chain.  A reverse step of the _resample entry points draws exactly as
 *     dd_sample_steps_fixed does, but with Philox counter word 2 = t + 65536 * epoch instead of t (epoch 0: the same bits).  The
 *     jump that raises the epoch to e draws at word 2 = m + 65536 * e on streams of its own -- 3 atom types, 4 bond types,
 *     8 coordinates (1, 2, 7 are the step's) -- with rows and keys addressed exactly like the step's: seed and flat row, or
 *     sample_keys[b] and the row of the sample's own enumeration.  So sample_keys keeps its promise under resampling.
 *     Needs T <= 65535 and at most 65535 jumps.
 *   dd_sampler_reset_resample: dd_sampler_reset and *epoch = 0; in front of every chain.
 * tab and epoch are DEVICE pointers read at every launch; jump_length is an argument of the jump launch only: a graph from
 * dd_graph_create_resample serves every chain of its shape and mode, whatever the mask, the keys, jump_length and the number of
 * passes (dd_graph_launch / dd_graph_destroy take it like any other).  `size` is the caller's sizeof(dd_resample).
 *   resample == NULL, fixed == NULL, jump_length < 1, a NULL tab / epoch, T > 65535, injected noise (s->u_v / u_b / eps), and for
 *   the jump a dd_fixed without cc: DD_ERR_BAD_ARG before any launch.  (New entry points, ABI unchanged.) */
typedef struct dd_resample {
  int32_t size;                  /* sizeof(dd_resample) of the caller */
  int32_t jump_length;           /* j >= 1 */
  const float* tab;              /* DEVICE [6][T] */
  int32_t* epoch;                /* DEVICE [1] */
} dd_resample;
int dd_sample_steps_resample(const dd_sampler* s, const dd_model_opts* opts /*HOST*/, const uint64_t* sample_keys /*DEVICE [B] or NULL*/,
                             const dd_fixed* fixed /*HOST*/, const dd_resample* resample /*HOST*/, int n_steps, void* stream);
int dd_graph_create_resample(const dd_sampler* s, const dd_model_opts* opts /*HOST*/, const uint64_t* sample_keys /*DEVICE [B] or NULL*/,
                             const dd_fixed* fixed /*HOST*/, const dd_resample* resample /*HOST*/, int steps_per_graph, void* stream,
                             void** graph_out /*HOST*/);
int dd_resample_jump(const dd_sampler* s, const uint64_t* sample_keys /*DEVICE [B] or NULL*/, const dd_fixed* fixed /*HOST*/,
                     const dd_resample* resample /*HOST*/, void* stream);
int dd_sampler_reset_resample(const dd_sampler* s, const dd_resample* resample /*HOST*/, void* stream);

/* Chain init (EXTENSION): the chain's state in front of its first step, drawn on the device with the chain's own Philox
 * addressing, so that a keyed sample's STARTING POINT is as independent of its batch as its chain.  One launch (after
 * dd_sampler_reset, before dd_fixed_init and the first step) writes lig_pos (centred), lig_v and lig_bond of every REAL row;
 * padding rows of a padded batch (atoms >= nl_real[b], bond rows with such an endpoint) keep what the host put there.
 *   cc [B*NL,3] / std [B*NL,3]: per-atom centred centre (centre - offset of the sample) and std; they need not be the centres
 *     and atom_std the steps use.  atom_log_prior [num_v] / bond_log_prior [5]: log prior of the classes, NULL = the prior row
 *     of the chain's own table (tab_v / tab_b at 4 * T + c).
 *   DD_INIT_PRIOR: the level above the first step, drawn at Philox time word T:
 *       x = cc + (e * std)                 class = argmax_c gumbel(u_c) + log_prior_c     (uniform prior: the reference's
 *                                                                                          log_sample_categorical(zeros))
 *   DD_INIT_NOISED (partial diffusion): level l = t_start (the run state's) of the forward process of a KNOWN ligand
 *     x0c [B*NL,3] (centred) / v0 [B*NL] / b0 [B*NL*(NL-1)], drawn at Philox time word l with tab [2][T] as in dd_fixed:
 *       x = A[l] * (x0c - cc) + (S[l] * e) * std + cc
 *       class = argmax_c gumbel(u_c) + log_add_exp(log_onehot(v0)_c + log_cumprod[l], log_1m_cumprod[l] + log_prior_c)
 *     (decompdiff.py:436-455, transitions.py:146-150).  Every operation is rounded on its own; the argmax takes the first
 *     largest class.
 *   Draws: streams of their own -- 5 atom types, 6 bond types, 9 coordinates (class blocks as everywhere) -- with rows and keys
 *     addressed exactly like a step's: dd_sampler.seed and the flat row, or sample_keys[b] and the row of the sample's own
 *     enumeration.  No counter is shared with a step (1 / 2 / 7), a jump (3 / 4 / 8) or dd_fixed_init.
 * All pointers are DEVICE pointers; `size` is the caller's sizeof(dd_init).
 *   init == NULL, an unknown mode, a NULL cc / std, NOISED without x0c / v0 / b0 / tab or with t_start outside [0, T), injected
 *   noise (s->u_v / u_b / eps): DD_ERR_BAD_ARG before any launch.  (New entry point, ABI unchanged.) */
enum { DD_INIT_PRIOR = 1, DD_INIT_NOISED = 2 };
typedef struct dd_init {
  int32_t size;                  /* sizeof(dd_init) of the caller */
  int32_t mode;                  /* DD_INIT_PRIOR / DD_INIT_NOISED */
  const float* cc;               /* DEVICE [B*NL,3] */
  const float* std;              /* DEVICE [B*NL,3] */
  const float* atom_log_prior;   /* DEVICE [num_v] or NULL */
  const float* bond_log_prior;   /* DEVICE [5] or NULL */
  const float* x0c;              /* DEVICE [B*NL,3], NOISED only */
  const int32_t* v0;             /* DEVICE [B*NL], NOISED only */
  const int32_t* b0;             /* DEVICE [B*NL*(NL-1)], NOISED only */
  const float* tab;              /* DEVICE [2][T], NOISED only */
} dd_init;
int dd_chain_init(const dd_sampler* s, const uint64_t* sample_keys /*DEVICE [B] or NULL*/, const dd_init* init /*HOST*/, void* stream);

/* Drift guidance gradients at x_t (utils/guidance_funcs.py:24-78), analytic. grad [B,NL,3]. */
int dd_drift_armsca(const float* lig_pos, const int32_t* decomp_index, int B, int NL, float min_d, float max_d,
                    float* grad, int accumulate, void* stream);
int dd_drift_clash(const float* lig_pos, const float* offset, const float* full_protein_pos, int B, int NL, int NF,
                   float sigma, float gamma, float* grad, int accumulate, void* stream);
/* grad[B*NL,3] (+)= d/dx of compute_batch_arms_repul_loss (utils/guidance_funcs.py:94-118, :81-91) -- the torch.autograd.grad
 * of that energy: sum over the samples' arm pairs a1 <= a2 of relu(max_d - min distance) (mode 1 = 'min') or of the mean of
 * relu(max_d - distance) over all atom pairs (mode 2 = 'all'), divided by B.  decomp_index [B*NL]: -1 scaffold, >= 0 arm id. */
int dd_drift_arms_repul(const float* lig_pos, const int32_t* decomp_index, int B, int NL, float max_d, int mode, float* grad,
                        int accumulate, void* stream);

/* Distance restraints (EXTENSION; a fourth drift term with caller-supplied geometry -- pharmacophore points): restraint r belongs
 * to ONE sample and asks that an atom of it stays min_d_r .. max_d_r from the point p_r (min_d may be 0, max_d +inf), weight w_r >= 0:
 *     d_r = | x_w - p_r |      w = the explicit atom atom[r] (its row within the sample, 0 .. NL-1), or, atom[r] == -1, the FIRST
 *                              nearest member in row order (strict <) of the group group[r]: DD_RESTRAINT_ANY -- every real atom of
 *                              the sample (decomp_index is not read) --, -1 -- the scaffold (decomp_index == -1) --, a >= 0 -- arm a
 *     E   = sum_r  w_r * ( max(min_d_r - d_r, 0) + max(d_r - max_d_r, 0) )
 * No division by the batch size or by R: a sample's gradient does not depend on its batch.  The gradient is torch.autograd.grad(E, x):
 * the clamps pass theirs at exact equality with a bound (min_d == max_d == d: the two cancel), d == 0 gives nothing (finite), an
 * empty group -- an arm the sample does not have, every group but ANY without decomp_index -- gives nothing (distance +inf,
 * winner -1).  Padding atoms of a padded batch (row >= nl_real[b]) are never eligible.  Points are in the frame of lig_pos (the
 * host subtracts the sample's offset).  Restraints arrive sorted by sample: ptr [B+1] with ptr[0] == 0 and ptr[B] == R.
 *   dd_drift_restraint: grad [B*NL,3] (+)= dE/dx, every row written (zeros where nothing acts); optional dist [R] and winner [R]
 *     (row within the sample, or -1).  step_counter != NULL (a dd_sampler's run state): the term acts only while
 *     t_min <= t <= t_max, t the run state's current time, and writes zeros outside; dist / winner are reported either way.
 *     One workgroup per sample, no atomics: the same bits on every run.
 *   dd_sample_steps_guided / dd_graph_create_guided: the reverse steps of the _resample entry points with every extra NULL-able
 *     -- sample_keys, fixed, resample (needs fixed), restraints -- and the last of the suffix chain: the _resample pair forwards
 *     here.  The step subtracts the restraint gradient at x_t, times tab_score[t] when `scale`, from the posterior mean next to
 *     the other drift terms, inside the window only; held atoms take part as targets and their own motion is overwritten by the
 *     hold; a resampling jump and the chain init take no drift.  Every restraint pointer is a DEVICE pointer read at every launch:
 *     one graph serves any restraint values and any split of the R entries over the samples.  R, scale, t_min and t_max are
 *     arguments of the launches, so a graph keeps those of its creation (a host that varies the count pads to a capacity with
 *     weight-0 entries).  The gradient lives in the workspace (dd_workspace_floats grew by B*NL*3 floats, rounded up).
 *   `size` is the caller's sizeof(dd_restraints).  DD_ERR_BAD_ARG before any launch: NL > 128, R < 0, a NULL ptr (or, R > 0, any
 *   other NULL array), t_min > t_max, and -- read back from the device with one synchronous copy on `stream` -- a ptr that does
 *   not start at 0, rise monotonically and end at R, an atom outside [-1, NL), a group below -1 other than DD_RESTRAINT_ANY, an
 *   arm / scaffold group without decomp_index.  dd_reverse_step stays without restraints.  (New entry points, ABI unchanged.)
 *
 * The general form (typed atoms, ligand-ligand pairs, harmonic hinges, per-step distances) rides on the trailing fields of
 * dd_restraints, every one a NULL-able DEVICE pointer.  A struct whose `size` ends before them, or that leaves them all NULL,
 * is served by the kernel described above, bit for bit; any non-NULL one sends the launch to the general kernel.
 *   Endpoints: restraint r has endpoint 1 -- atom[r] / group[r], filtered by the class set cls[r] -- and, where pair[r] != 0,
 *     endpoint 2 -- atom2[r] / group2[r] / cls2[r]; without a pair its other end is point[r] as above.
 *   Candidates: an endpoint's candidates are the explicit atom or the real atoms of the group (never a padding row).  A class set
 *     is a 32-bit mask (bit c = class c; NULL array: untyped) and keeps the candidates whose CURRENT class lig_v[row] is in it:
 *     an explicit atom of another class is an empty set, a class id outside [0, 32) matches nothing.
 *   Point restraint: as above over the filtered set (first nearest in row order; empty: +inf, winner -1, no gradient).
 *   Pair restraint: the winner is the pair (i, j), i in set 1, j in set 2, i != j, that minimises d = |x_i - x_j|; ties go to the
 *     first in (i, then j) row order under strict <.  With u = (x_i - x_j) / d the gradient +c u goes on row i and -c u on row j,
 *     c the hinge coefficient of the form in force; d == 0 gives nothing; an empty set, or two sets that are the same single
 *     atom, give +inf / -1 / -1 and nothing.  point[r] of a pair is not read.
 *   Form: form[r] == 0 (or a NULL array), linear: w (relu(min_d - d) + relu(d - max_d)), c = -w / +w;  form[r] == 1, harmonic:
 *     w (relu(min_d - d)^2 + relu(d - max_d)^2), c = -2 w (min_d - d) below the window, 2 w (d - max_d) above it.  No division
 *     by B or R in either.  scale, t_min / t_max and weight >= 0 keep their meaning.
 *   Held atoms (dd_fixed) are candidates; the hold overwrites their own motion: of a pair with one held end only the free end moves.
 *   Trajectories: with a run state, every launch writes row `step` (steps done) of dist_traj / winner_traj / winner2_traj
 *     [traj_positions, R] -- the distance and winner(s) at the state the step of that position takes its gradient from --,
 *     window open or not; nothing is written at step >= traj_positions or without a run state.
 *   dd_drift_restraint2: dd_drift_restraint with the atom classes lig_v (NULL: untyped only) and winner2 [R] (the j of a pair; -1
 *     for a point restraint or an empty pair).  dd_sample_steps_guided / dd_graph_create_guided pass the sampler's own lig_v.
 *   One workgroup per sample, no atomics: the same bits on every run, and a sample's rows do not depend on its batch.
 *   DD_ERR_BAD_ARG before any launch, beyond the list above: pair without atom2 and group2; for a pair row an atom2 outside
 *   [-1, NL), or, atom2 == -1, a group2 that is neither DD_RESTRAINT_ANY nor >= -1 (DD_RESTRAINT_NONE included), or an arm /
 *   scaffold group2 without decomp_index; a form outside {0, 1}; cls / cls2 with a NULL lig_v; trajectory pointers with
 *   traj_positions <= 0.  dd_drift_restraint itself refuses a struct that carries any of the trailing arrays. */
enum { DD_RESTRAINT_ANY = -3 };  /* not an arm id (>= 0), not the scaffold (-1), not the padding mark of padded chains (-2) */
enum { DD_RESTRAINT_NONE = -4 }; /* group2 of a row without a second endpoint: matches no atom */
typedef struct dd_restraints {
  int32_t size;                  /* sizeof(dd_restraints) of the caller */
  int32_t R;                     /* restraints in the arrays */
  const int32_t* ptr;            /* DEVICE [B+1] */
  const float* point;            /* DEVICE [R,3] */
  const float* min_d;            /* DEVICE [R] */
  const float* max_d;            /* DEVICE [R] */
  const float* weight;           /* DEVICE [R] */
  const int32_t* atom;           /* DEVICE [R] */
  const int32_t* group;          /* DEVICE [R] */
  int32_t scale;                 /* != 0: the step multiplies the gradient by tab_score[t] */
  int32_t t_min, t_max;          /* the window, inclusive (0 and T - 1: always) */
  /* the general form: every field below may be NULL / 0, and a caller's smaller `size` reads as that */
  const uint32_t* cls;           /* DEVICE [R] class mask of endpoint 1 */
  const uint32_t* cls2;          /* DEVICE [R] class mask of endpoint 2 */
  const int32_t* pair;           /* DEVICE [R] != 0: a pair restraint */
  const int32_t* atom2;          /* DEVICE [R] */
  const int32_t* group2;         /* DEVICE [R] */
  const int32_t* form;           /* DEVICE [R] 0 linear, 1 harmonic */
  float* dist_traj;              /* DEVICE [traj_positions, R] */
  int32_t* winner_traj;          /* DEVICE [traj_positions, R] row within the sample or -1 */
  int32_t* winner2_traj;         /* DEVICE [traj_positions, R] */
  int32_t traj_positions;        /* rows of the trajectory buffers */
} dd_restraints;
int dd_drift_restraint(const float* lig_pos, const int32_t* decomp_index /*or NULL*/, const int32_t* nl_real /*or NULL*/, int B, int NL,
                       const dd_restraints* restraints /*HOST*/, const int32_t* step_counter /*DEVICE [4] or NULL*/, float* grad,
                       int accumulate, float* dist /*or NULL*/, int32_t* winner /*or NULL*/, void* stream);
int dd_drift_restraint2(const float* lig_pos, const int32_t* lig_v /*int32 [B*NL] or NULL: untyped only*/, const int32_t* decomp_index /*or NULL*/,
                        const int32_t* nl_real /*or NULL*/, int B, int NL, const dd_restraints* restraints /*HOST*/,
                        const int32_t* step_counter /*DEVICE [4] or NULL*/, float* grad, int accumulate, float* dist /*or NULL*/,
                        int32_t* winner /*or NULL*/, int32_t* winner2 /*or NULL*/, void* stream);
int dd_sample_steps_guided(const dd_sampler* s, const dd_model_opts* opts /*HOST*/, const uint64_t* sample_keys /*DEVICE [B] or NULL*/,
                           const dd_fixed* fixed /*HOST or NULL*/, const dd_resample* resample /*HOST or NULL*/,
                           const dd_restraints* restraints /*HOST or NULL*/, int n_steps, void* stream);
int dd_graph_create_guided(const dd_sampler* s, const dd_model_opts* opts /*HOST*/, const uint64_t* sample_keys /*DEVICE [B] or NULL*/,
                           const dd_fixed* fixed /*HOST or NULL*/, const dd_resample* resample /*HOST or NULL*/,
                           const dd_restraints* restraints /*HOST or NULL*/, int steps_per_graph, void* stream, void** graph_out /*HOST*/);

/* Build flags of the loaded library: bit 0 = measurement build (-DDD_DEBUG_OPTIONS=1: alternative launch schedules behind
 * dd_debug_set_option, see decompdiff_hip_debug.h), bit 1 = -DDD_EXACT_MATH=1 (correctly rounded 1/sqrt and softmax
 * division).  0 for the default library. */
int dd_build_flags(void);

/* Measurement, profiling and test-access entry points (dd_profile_step, dd_debug_*, dd_queue_error, dd_workspace_view)
 * are declared in decompdiff_hip_debug.h: exported by the same library, not part of the drop-in boundary. */

#ifdef __cplusplus
}
#endif
#endif /* DECOMPDIFF_HIP_H */
