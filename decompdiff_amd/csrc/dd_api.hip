// C ABI orchestration: workspace carving, the score-network forward (launch sequence of
// models/decompdiff.py:213-351 + uni_transformer_edge.py:259-287,394-443) and the reverse loop
// (decompdiff.py:575-689), eager or as a replayed hipGraph.
#include <mutex>
#include <thread>
#include <vector>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include <string>
#include <sys/stat.h>
#include <unistd.h>

#include "dd_kernels.hpp"

namespace dd {

// ---- workspace --------------------------------------------------------------------------------
struct Workspace {
  float *xa, *xb, *h, *hb, *ew, *P, *PL, *PB, *P2, *PL2, *PB2, *Ek, *Ev, *Rk, *Rv, *q1bl, *qn, *ql, *ql2, *qlnb, *qb, *A, *Anb, *dxe, *dxb, *ga, *gc, *gr, *gq, *h2, *hs;
  int32_t* nbr;
  int32_t* counters;       // [64] work counters of the persistent attention workgroups (one per layer), zeroed per forward
  size_t total;
};

static inline size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }

static Workspace carve(float* base, int B, int NP, int NL, int K) {
  Workspace w;
  const size_t N = (size_t)NP + NL, Eb = (size_t)NL * (NL > 0 ? NL - 1 : 0);
  size_t off = 0;
  auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += align64(n); return p; };
  w.xa = take(B * N * 3);
  w.xb = take(B * N * 3);
  w.h = take(B * N * 128);
  w.hb = take(B * Eb * 128);
  w.nbr = reinterpret_cast<int32_t*>(take(B * N * K));
  w.ew = take(B * N * K);
  w.P = take(B * N * 640);
  w.PL = take((size_t)B * NL * 1280);
  w.PB = take(B * Eb * 640);
  w.P2 = take(B * N * 256);
  w.PL2 = take((size_t)B * NL * 1024);
  w.PB2 = take(B * Eb * 256);
  w.Ek = take(B * Eb * 128);
  w.Ev = take(B * Eb * 128);
  w.Rk = take(B * Eb * 128);
  w.Rv = take(B * Eb * 128);
  w.q1bl = take(B * Eb * 128);
  w.qn = take(B * N * 128);
  w.ql = take((size_t)B * NL * 128);
  w.ql2 = take((size_t)B * NL * 128);
  w.qlnb = take((size_t)B * NL * 128);
  w.qb = take(B * Eb * 128);
  w.A = take(B * N * 128);
  w.Anb = take((size_t)B * NL * 128);
  w.dxe = take((size_t)B * NL * 3);
  w.dxb = take((size_t)B * NL * 3);
  w.ga = take((size_t)B * NL * 3);
  w.gc = take((size_t)B * NL * 3);
  w.gr = take((size_t)B * NL * 3);
#if defined(DD_DEBUG_OPTIONS) && DD_DEBUG_OPTIONS          // (measurement build: the one-fork-per-layer schedule, option 27)
  w.h2 = take(B * N * 128);                              // ping-pong partner of h / the side stream's own copy of the new h
  w.hs = take(B * N * 128);
#else
  w.h2 = w.hs = nullptr;                                 // the shipped schedule never reads them (g_side_lin is the constant 0)
#endif
  w.counters = reinterpret_cast<int32_t*>(take(DD_NUM_COUNTERS + DD_NUM_FLAGS));   // (+ the layer-tail queue's flag words)
  w.gq = take((size_t)B * NL * 3);                       // restraint gradient (last: every earlier buffer keeps its offset)
  w.total = off;
  return w;
}

static inline int num_v(const dd_sampler* s) { return s->num_v > 0 ? s->num_v : DD_NUM_V; }

// Rows of the ligand projection W_l1, read from the HOST slot table (include/decompdiff_hip.h, slot_off): b_l1 follows W_l1, so
// their distance is rows * 128 floats -- 1280 rows for the wide bond layer (h_node_in_bond_net: True), 640 for the narrow one
// (both multiples of the arena's 64-float slot padding, so the difference is exact).  0: another size, or layers that disagree.
static int l1_rows(const dd_sampler* s) {
  int rows = 0;
  for (int l = 0; l < s->num_layers; ++l) {
    const int64_t* off = s->slot_off + (long)l * DD_NUM_LAYER_SLOTS;
    const int64_t d = off[DD_b_l1] - off[DD_W_l1];
    if ((d != 640 * 128 && d != 1280 * 128) || (l > 0 && d != (int64_t)rows * 128)) return 0;
    rows = (int)(d / 128);
  }
  return rows;
}

static int check_shapes(const dd_sampler* s) {
  if (!s || !s->weights || !s->slot_off || !s->workspace) return DD_ERR_BAD_ARG;
  if (s->B <= 0 || s->NP < 0 || s->NL < 2 || s->K <= 0 || s->num_layers < 1 || s->num_layers > 64) return DD_ERR_BAD_ARG;
  if (l1_rows(s) == 0) return DD_ERR_BAD_ARG;
  const int N = s->NP + s->NL;
  if (s->NL > DD_NL_MAX || N > DD_N_MAX || s->K > DD_KNN_MAX || s->K > N - 1) return DD_ERR_UNSUPPORTED_SHAPE;
  if (s->num_v != 0 && s->num_v != 8 && s->num_v != 13 && s->num_v != 23) return DD_ERR_UNSUPPORTED_SHAPE;   // utils/transforms.py:138-151
  if (num_v(s) != DD_NUM_V && s->l0_tables != nullptr) return DD_ERR_BAD_ARG;
  if (s->workspace_floats < dd_workspace_floats(s->B, s->NP, s->NL, s->K)) return DD_ERR_WORKSPACE_TOO_SMALL;
  if ((s->nl_real != nullptr) != (s->bl_prefix != nullptr) || (s->np_real != nullptr && s->nl_real == nullptr)) return DD_ERR_BAD_ARG;
  return DD_OK;
}

// ---- optional per-category HIP-event profiler (dd_profile_forward) --------------------------------
struct Profiler {
  static constexpr int MAXEV = 512;
  hipEvent_t start[MAXEV], stop[MAXEV];
  int cat[MAXEV];
  int n = 0, created = 0;
};
static Profiler* g_prof = nullptr;

struct ProfScope {
  hipStream_t st; int idx;
  ProfScope(int cat, hipStream_t s, bool on = true) : st(s), idx(-1) {
    if (on && g_prof && g_prof->n < Profiler::MAXEV) {
      idx = g_prof->n++;
      g_prof->cat[idx] = cat;
      (void)hipEventRecord(g_prof->start[idx], st);
    }
  }
  ~ProfScope() { if (idx >= 0) (void)hipEventRecord(g_prof->stop[idx], st); }
};
#define DD_TRYP(cat, expr)               \
  do {                                  \
    ProfScope prof_scope__(cat, st);    \
    int rc__ = (expr);                  \
    if (rc__ != DD_OK) return rc__;     \
  } while (0)

#define DD_TRY(expr)            \
  do {                          \
    int rc__ = (expr);          \
    if (rc__ != DD_OK) return rc__; \
  } while (0)

// second stream for the coordinate sub-layers (they only feed the NEXT layer's geometry, so they overlap its
// projection GEMMs); fork/join through events, which stream capture turns into graph edges
extern int g_gemm_ksplit;                      // dd_gemm.hip
#if defined(DD_DEBUG_OPTIONS) && DD_DEBUG_OPTIONS
extern int g_tail_variant;
#endif
static bool g_gemm_ksplit_on() { return g_gemm_ksplit != 0; }   // (the addend form above lives in the K-split tile)
// Side stream and fork / join events, one set per device (a process may drive several devices; multi-GPU runs use one
// process per GPU, where this is a single entry).  They only shape a graph while it is being captured, and captures are
// serialised by g_capture_mutex, so one set per device is enough for any number of samplers.
struct DevCtx {
  hipStream_t side = nullptr;
  hipEvent_t ev_qa_fork[8], ev_qb_fork[8], ev_fork[9], ev_join[9];   // per-layer events: slot (step & 7), see forward_impl
};
static DevCtx g_dev_ctx[16];
static std::mutex g_capture_mutex;
static DevCtx& dev_ctx() {                       // (fetched once at the top of a forward)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
  return g_dev_ctx[dev];
}
// Launch-schedule / kernel alternatives kept for A/B measurements (EXPERIMENTS.md).  They exist only in the measurement
// build (`python -m decompdiff_amd.build --debug-options` -> lib/libdecompdiff_hip_dbg.so, -DDD_DEBUG_OPTIONS=1, selected
// with DD_HIP_LIB); in the default library the values below are compile-time constants, the alternative paths are not
// compiled, and dd_debug_set_option only knows key 0 (one launch per sub-layer: the cross-check).
#ifndef DD_SIDE_LIN_DEFAULT
#define DD_SIDE_LIN_DEFAULT 0
#endif
#if defined(DD_DEBUG_OPTIONS) && DD_DEBUG_OPTIONS
#define DD_OPT static int
#else
#define DD_OPT static constexpr int
#endif
DD_OPT g_step_fused = 1;                   // dd_debug_set_option(7, v): rows + coordinates + counter in one launch
DD_OPT g_step_fold = 1;                    // dd_debug_set_option(20, v): step boundary folded (counter advanced by the forward's
                                               // first launch; last x update + x0 extraction inside the step kernel)
DD_OPT g_xup_in_asm = 1;                   // dd_debug_set_option(19, v): x += dx applied by the next layer's assemble launch
DD_OPT g_sched = 4;                        // dd_debug_set_option(8, v): 5 = tile queues with in-launch hand-offs (forward_tail;
                                               // measured slower, EXPERIMENTS.md round 3); 0 = coordinate sub-layers on the side stream,
                                               // 1 = next layer's projections ahead on the side stream, 2 = the same in two
                                               // launches (bond part forked at the node attention), 3 (-3 % in the
                                               // in-process A/B) = 2 + the next layer's query GEMMs on the side stream too,
                                               // 4 (default, another -2 %) = 3 with two joins: assemble waits for the
                                               // projections only and runs beside the query GEMMs, which are joined at the
                                               // node attention
DD_OPT g_xup_in_pos = 0;                   // dd_debug_set_option(11, v): x update inside the coordinate launch (last workgroup);
                                               // measured 1 % slower than the separate 3-block launch, off
DD_OPT g_fused_max_nl = DD_NL_MAX;                // dd_debug_set_option(13, v): largest ligand handled by the fused launches
DD_OPT g_defer_pos = 0;                    // dd_debug_set_option(14, v): record the coordinate launch after the next layer's GEMMs
                                               // (keeps the GEMM chain on the main queue; measured 1.3 % slower: the coordinate
                                               // launch then starves behind the projections' workgroups)
DD_OPT g_lin_with_pb2 = 1;                 // dd_debug_set_option(16, v): bond projections of the coordinate sub-layer ride with lin_node
DD_OPT g_pb_early = 1;                     // dd_debug_set_option(17, v): next layer's bond projections in the lin_node launch
DD_OPT g_q1_in_gemm = 1;                   // dd_debug_set_option(12, v): bond-layer query hidden row summed inside the query GEMM
DD_OPT g_l0_tables = 1;                    // dd_debug_set_option(22, v): first layer's projection / query rows gathered from tables
DD_OPT g_head_fused = 1;                   // dd_debug_set_option(24, v): head of a forward in two launches (0 = four, the cross-check)
DD_OPT g_side_lin = DD_SIDE_LIN_DEFAULT;   // dd_debug_set_option(27, v): ONE fork per layer -- the side stream forms the new h itself
                                               // (a second, identical lin_node launch into its own buffer) instead of waiting for the
                                               // main stream's lin_node, whose launch then has no cross-queue successor
// lin_node (h += W_lin . A + b) inside the NE / NB blocks of the node launch (round 6): no lin_node launch on the layer's critical
// chain, one fork per layer instead of two.  -1 = by shape (lin_in_node_for): measured -7 % step time at B = 1 and +4 % at B = 8, where
// the side stream's GEMM chain is the longer branch either way and the node launch pays ~9 us for the extra phase (EXPERIMENTS.md
// R6-3); DD_LIN_IN_NODE=0/1 or dd_debug_set_option(32, v) force it.
static int g_lin_in_node = [] { const char* e = getenv("DD_LIN_IN_NODE"); return e ? (e[0] == '1' ? 1 : (e[0] == '0' ? 0 : -1)) : -1; }();
// ... and with it the next layer's node projections ride in the main stream's projection launch (the side stream keeps the bond
// projections and the query GEMMs): DD_LIN_PROJ_MAIN=0/1
static int g_lin_proj_main = [] { const char* e = getenv("DD_LIN_PROJ_MAIN"); return e ? (e[0] == '1' ? 1 : 0) : 0; }();
static bool lin_in_node_for(int B, int NL) {
  if (g_lin_in_node >= 0) return g_lin_in_node != 0;
  return (long)B * NL * (NL - 1) < 8L * 256 * 2;        // fewer than two bond-layer trips per CU: the launch chain, not the node launch, bounds the step
}
DD_OPT g_head_rows_first = 0;              // dd_debug_set_option(29, v): see the head of forward_impl
DD_OPT g_heads_early = 1;                  // dd_debug_set_option(28, v): heads' first Linear in the last layer's projection launch
// Does this forward run lin_node inside the node launch?  (out_fc: the in-kernel lin_node has no node-output stage; fused: the
// one-launch-per-sub-layer loop has no such launch.)  Asked by the layer loop, the heads at the tail and dd_workspace_view.
static bool uses_lin_in_node(int B, int NL, bool out_fc, bool fused) {
  return fused && !out_fc && lin_in_node_for(B, NL) && g_lin_with_pb2 && !g_side_lin && g_heads_early;
}
DD_OPT g_q_in_pos = 1;                     // dd_debug_set_option(9, v): coordinate query MLPs' second layer inside attn_pos
extern int g_pos_waves;                     // dd_attention2.hip: waves per workgroup of the coordinate launch
DD_OPT g_p2_in_pos = 0;                    // dd_debug_set_option(30, v): the projections of the new h ({P2, PL2}; in the last layer the
                                               // heads' first Linear too) run in the leading / trailing workgroups of the coordinate
                                               // launch instead of a launch of their own on the critical chain (round 5: bit-identical,
                                               // measured 2.6 % SLOWER -- 40 us where the two launches take 11 + 23; EXPERIMENTS.md R5-2)
// (ev_fork / ev_join: [0..7] per layer, [8] graph construction at the head of a forward)
// DD_SIDE_PRIO: 0 (default since round 6) default priority for the side stream, 1 lowest (rounds 3-6), 2 highest.  A stream of another
// priority takes its hardware queue from a pool of its own (ROCm keeps GPU_MAX_HW_QUEUES = 4 queues PER PRIORITY); with it the process
// could reach a fifth active queue as soon as a second step graph was instantiated, and every graph from then on ran 14 % (B = 8) to 42 %
// (B = 1) slower -- the same slowdown GPU_MAX_HW_QUEUES >= 5 causes for the first graph.  At the default priority all of the process's
// streams share the four queues (EXPERIMENTS.md R6-11; tools/two_lengths.py).
static int g_side_low_priority = [] { const char* e = getenv("DD_SIDE_PRIO"); return (e && e[0] == '1') ? 1 : ((e && e[0] == '2') ? 2 : 0); }();
static int g_overlap = 1;                     // measured in-process A/B: -3.5 % step time
static int ensure_side_stream(DevCtx& dc) {
  if (dc.side) return DD_OK;
  {
    int lo = 0, hi = 0;                                  // (DD_SIDE_PRIO=1: lowest priority -- side work fills CUs the main chain leaves idle)
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = 0; (void)hipGetLastError(); }
    if (hipStreamCreateWithPriority(&dc.side, hipStreamNonBlocking, g_side_low_priority == 1 ? lo : (g_side_low_priority == 2 ? hi : 0)) != hipSuccess) return DD_ERR_HIP;
  }
  for (int i = 0; i < 8; ++i)
    if (hipEventCreateWithFlags(&dc.ev_qa_fork[i], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&dc.ev_qb_fork[i], hipEventDisableTiming) != hipSuccess)
      return DD_ERR_HIP;
  for (int i = 0; i < 9; ++i)
    if (hipEventCreateWithFlags(&dc.ev_fork[i], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&dc.ev_join[i], hipEventDisableTiming) != hipSuccess)
      return DD_ERR_HIP;
  return DD_OK;
}

static int g_fuse = 1;                       // dd_debug_set_fusion: 0 = one launch per sub-layer (per-kernel timing)
extern long long* g_gemm_dbg;              // dd_gemm.hip
extern long long* g_node_trace;            // dd_attention2.hip
static long long* g_dbg_clock = nullptr;   // set by dd_debug_set_clock_buffer (profiling aid)
static int g_dbg_mode = -1;


static int attn_dispatch(int mode, const AttnArgs& a0, hipStream_t st) {
  AttnArgs a = a0;
  a.dbg_clock = (mode == g_dbg_mode) ? g_dbg_clock : nullptr;
  return launch_attn2(mode, a, st);
}

// What one_step hands from the forward to the step kernels when the step boundary is folded (option 20).
struct StepFold {
  bool advance = false;                  // in: let the forward's first launch advance the step counter
  bool fold_tail = false;                // in: leave the last coordinate update + x0 extraction to the step kernel
  const float* xprev = nullptr;          // out: != nullptr when the tail was deferred
};

// Distance-aware bond head ('pre_att', decompdiff.py:323-341; include/decompdiff_hip.h dd_bond_head): the hidden row of
// ligand bond e = (src, dst) of the dst-major bond list,
//   out[e] = W_r^T exp(coeff (d - offset)^2) + P[dst] + P[src] + b1,   d = |x_dst - x_src| of the FINAL coordinates,
// where P = (W1_h / 2) h is one GEMM row per ligand atom (rows b * NL + i, launched in front of this one).  The final ligand
// coordinates are x[b, NP + i] -- plus dxe + dxb when the last coordinate update is still pending (the folded step tail; the
// same association as k_xupdate and the step kernel's x0).  One wave per bond, two hidden channels per lane; W_r, b1 and the
// centres stay in registers for all bonds of a wave.  Bonds with an endpoint at or beyond nl_real[b] (padding atoms of a
// padded batch) get a zero row.
__global__ __launch_bounds__(256) void k_bond_head_pre_att(const float* __restrict__ P, const float* __restrict__ x,
                                                           const float* __restrict__ dxe, const float* __restrict__ dxb, int NP, int NL,
                                                           const float* __restrict__ W_r, const float* __restrict__ b1,
                                                           const float* __restrict__ offset, float coeff,
                                                           const int32_t* __restrict__ nl_real, long rows, float* __restrict__ out) {
  constexpr int G = 20;
  const int lane = threadIdx.x & 63;
  const long nwaves = (long)gridDim.x * 4;
  float2 wr[G];
  float c[G];
#pragma unroll
  for (int k = 0; k < G; ++k) {
    wr[k] = *reinterpret_cast<const float2*>(W_r + k * 128 + 2 * lane);
    c[k] = offset[k];
  }
  const float2 bb = *reinterpret_cast<const float2*>(b1 + 2 * lane);
  const int N = NP + NL, NLm1 = NL - 1;
  const long Eb = (long)NL * NLm1;
  for (long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6); e < rows; e += nwaves) {
    const int b = (int)(e / Eb);
    const int r = (int)(e - (long)b * Eb);
    const int t = r / NLm1, sp = r - t * NLm1;
    const int src = sp + (sp >= t);
    float2* o = reinterpret_cast<float2*>(out + e * 128 + 2 * lane);
    if (nl_real != nullptr && (t >= nl_real[b] || src >= nl_real[b])) {
      *o = make_float2(0.f, 0.f);
      continue;
    }
    float xd[3], xs[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      xd[q] = x[((long)b * N + NP + t) * 3 + q];
      xs[q] = x[((long)b * N + NP + src) * 3 + q];
      if (dxe != nullptr) {
        const long id = ((long)b * NL + t) * 3 + q, is = ((long)b * NL + src) * 3 + q;
        xd[q] = xd[q] + dxe[id] + dxb[id];
        xs[q] = xs[q] + dxe[is] + dxb[is];
      }
    }
    const float dx = xd[0] - xs[0], dy = xd[1] - xs[1], dz = xd[2] - xs[2];
    const float d = sqrtf(dx * dx + dy * dy + dz * dz);
    const float2 pd = *reinterpret_cast<const float2*>(P + ((long)b * NL + t) * 128 + 2 * lane);
    const float2 ps = *reinterpret_cast<const float2*>(P + ((long)b * NL + src) * 128 + 2 * lane);
    float2 acc = make_float2(bb.x + (pd.x + ps.x), bb.y + (pd.y + ps.y));
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const float u = d - c[k];
      const float g = expf(coeff * (u * u));
      acc.x = fmaf(wr[k].x, g, acc.x);
      acc.y = fmaf(wr[k].y, g, acc.y);
    }
    *o = acc;
  }
}

static bool is_pre_att(const dd_bond_head* bh) { return bh != nullptr && bh->kind == DD_BOND_HEAD_PRE_ATT; }

static int check_bond_head(const dd_bond_head* bh) {
  if (bh == nullptr || bh->kind == DD_BOND_HEAD_LIN) return DD_OK;
  if (bh->kind != DD_BOND_HEAD_PRE_ATT || bh->num_r != 20 || !bh->W_p || !bh->W_r || !bh->b1 || !bh->offset) return DD_ERR_BAD_ARG;
  return DD_OK;
}

// hidden rows of the pre_att head into w.qb from P (w.P) and the final coordinates (see k_bond_head_pre_att)
static int launch_bond_head_pre_att(const dd_sampler* s, const Workspace& w, const dd_bond_head* bh, const float* x, const float* dxe,
                                    const float* dxb, int NP, hipStream_t st) {
  const long rows = (long)s->B * s->NL * (s->NL - 1);
  const long blocks = (rows + 15) / 16;                 // (four bonds per wave)
  hipLaunchKernelGGL(k_bond_head_pre_att, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, w.P, x, dxe, dxb, NP,
                     s->NL, bh->W_r, bh->b1, bh->offset, bh->coeff, s->nl_real, rows, w.qb);
  DD_CHECK_LAUNCH();
  return DD_OK;
}

// ---- forward context: where every launch's arguments are defined -----------------------------------------------------------
// Jobs of up to six GEMMs for one launch_gemm128_batch call, appended one by one.
struct GemmList {
  GemmArgs j[6];
  int n = 0;
  void add(const GemmArgs& g) { j[n++] = g; }
  int launch(hipStream_t st) const { return launch_gemm128_batch(j, n, st); }
};

// g with W_lin . A_nb (still pending on the ligand rows of the h it reads) added to its X rows: all nodes of the batch (ligand
// rows n >= NP take row n - NP of their sample) or the ligand rows only.  anb == NULL: nothing is pending, g as it is.
static GemmArgs add_anb(GemmArgs g, const float* anb, bool all_nodes, int NP, int NL) {
  if (anb) { g.X2 = anb; g.x2_N = all_nodes ? NP + NL : NL; g.x2_NP = all_nodes ? NP : 0; }
  return g;
}

// What the sampler, the carved workspace and the shape say about each launch of a forward: one builder per GEMM job and per
// attention sub-layer of the network.  The schedules (forward_impl's two loops, forward_tail) only decide which jobs share a
// launch, on which stream, in which order, and set the few fields that depend on that.
struct Fwd {
  const dd_sampler* s;
  Workspace w;
  int B, NP, NL, K, N, nE;
  long Eb, hN;
  // bond-layer width, read once per call (l1_rows; the entry points refuse anything but 640 / 1280 in check_shapes).  Narrow: the
  // l1 launch forms the 640 node_layer_with_bond columns only -- w.PL keeps its 1280-float row stride and the workspace its
  // layout, columns [640, 1280) are neither written nor read -- the assemble launch adds no atom rows, and the bond-layer query
  // MLP's hidden row is PB.q_hb as it stands (no q1 block, no x2_sum epilogue).
  int plw;
  bool narrow;
  explicit Fwd(const dd_sampler* s_)
      : s(s_), w(carve(s_->workspace, s_->B, s_->NP, s_->NL, s_->K)), B(s_->B), NP(s_->NP), NL(s_->NL), K(s_->K), N(s_->NP + s_->NL),
        nE((int)((long)s_->B * s_->NL * (s_->NL - 1))), Eb((long)s_->NL * (s_->NL - 1)), hN((long)(s_->NP + s_->NL) * 128),
        plw(l1_rows(s_)), narrow(plw == 640) {}
  // (l: the step of the forward -- block b, layer l % num_layers of it: the blocks of a refine net share their weights)
  const float* LW(int l, int slot) const { return s->weights + s->slot_off[(long)(l % s->num_layers) * DD_NUM_LAYER_SLOTS + slot]; }
  const float* GW(int slot) const { return s->weights + s->slot_off[(long)s->num_layers * DD_NUM_LAYER_SLOTS + slot]; }
  GemmArgs add_anb(const GemmArgs& g, const float* anb, bool all_nodes) const { return dd::add_anb(g, anb, all_nodes, NP, NL); }
  float* anb_buf(int l) const { return (l & 1) ? w.A : w.Anb; }   // lin_in_node: where layer l's NB blocks leave W_lin . A_nb

  // -- first Linear of the node / bond sub-layers' MLPs from h / h_bond: columns [col0, col0 + ncols) of the 640-wide n1 and b1 rows
  //    (forward_tail forms the query-hidden block [512, 640) ahead of the rest), all 1280 of l1 (ligand rows of h)
  GemmArgs n1(int l, const float* h, int col0 = 0, int ncols = 640) const {
    return gemm_args(h, B * N, 0, 128, B * N, LW(l, DD_W_n1) + col0 * 128, LW(l, DD_b_n1) + col0, nullptr, w.P + col0, B * N, 0, 640, ncols, 0);
  }
  // (dd_layer0_prepare: the protein rows of layer 0 alone, static per chain, mapped into the [B, N] table s->l0_P)
  GemmArgs n1_l0_protein() const {
    return gemm_args(s->protein_h, NP, (long)NP * 128, 128, B * NP, LW(0, DD_W_n1), LW(0, DD_b_n1), nullptr, s->l0_P, NP, (long)N * 640, 640, 640, 0);
  }
  GemmArgs l1(int l, const float* h) const {
    return gemm_args(h + (long)NP * 128, NL, hN, 128, B * NL, LW(l, DD_W_l1), LW(l, DD_b_l1), nullptr, w.PL, B * NL, 0, 1280, plw, 0);
  }
  GemmArgs b1(int l, int col0 = 0, int ncols = 640) const {
    return gemm_args(w.hb, nE, 0, 128, nE, LW(l, DD_W_b1) + col0 * 128, LW(l, DD_b_b1) + col0, nullptr, w.PB + col0, nE, 0, 640, ncols, 0);
  }
  // -- the same for the coordinate sub-layers, from the new h / h_bond
  GemmArgs n2(int l, const float* h) const {
    return gemm_args(h, B * N, 0, 128, B * N, LW(l, DD_W_n2), LW(l, DD_b_n2), nullptr, w.P2, B * N, 0, 256, 256, 0);
  }
  GemmArgs l2(int l, const float* h) const {
    return gemm_args(h + (long)NP * 128, NL, hN, 128, B * NL, LW(l, DD_W_l2), LW(l, DD_b_l2), nullptr, w.PL2, B * NL, 0, 1024, 1024, 0);
  }
  GemmArgs b2(int l) const { return gemm_args(w.hb, nE, 0, 128, nE, LW(l, DD_W_b2), LW(l, DD_b_b2), nullptr, w.PB2, nE, 0, 256, 256, 0); }
  // -- query MLPs, second Linear (LayerNorm + ReLU prologue).  Bond layer: the hidden row is q_hb[bond] + q_hi[destination atom],
  //    summed while the tile stages its rows (x2_sum), or read from w.q1bl where the assemble launch left the sum.
  //    Narrow bond layer: q_hb[bond] alone, read in place whatever x2_sum says
  GemmArgs q_bl(int l, bool x2_sum) const {
    const bool in_pb = x2_sum || narrow;
    GemmArgs g = gemm_args(in_pb ? w.PB + 512 : w.q1bl, nE, 0, in_pb ? 640 : 128, nE, LW(l, DD_BL_W2q), LW(l, DD_BL_b2q), LW(l, DD_BL_lnq),
                           w.qb, nE, 0, 128, 128, 0);
    if (x2_sum && !narrow) { g.X2 = w.PL + 1152; g.x2_N = NL; g.x2_Eb = (int)Eb; g.x2_NLm1 = NL - 1; g.x2_ld = 1280; }
    return g;
  }
  GemmArgs q_ne(int l) const {
    return gemm_args(w.P + 512, B * N, 0, 640, B * N, LW(l, DD_NE_W2q), LW(l, DD_NE_b2q), LW(l, DD_NE_lnq), w.qn, B * N, 0, 128, 128, 0);
  }
  GemmArgs q_ne_l0_protein() const {                     // (the same rows' node queries, s->l0_P -> s->l0_qn)
    return gemm_args(s->l0_P + 512, NP, (long)N * 640, 640, B * NP, LW(0, DD_NE_W2q), LW(0, DD_NE_b2q), LW(0, DD_NE_lnq), s->l0_qn, NP,
                     (long)N * 128, 128, 128, 0);
  }
  GemmArgs q_nb(int l) const {
    return gemm_args(w.PL + 512, B * NL, 0, 1280, B * NL, LW(l, DD_NB_W2q), LW(l, DD_NB_b2q), LW(l, DD_NB_lnq), w.qlnb, B * NL, 0, 128, 128, 0);
  }
  // (coordinate sub-layers: only where the coordinate launch does not evaluate them itself, see q_in_pos)
  GemmArgs q_pe(int l) const {
    return gemm_args(w.PL2 + 256, B * NL, 0, 1024, B * NL, LW(l, DD_PE_W2q), LW(l, DD_PE_b2q), LW(l, DD_PE_lnq), w.ql, B * NL, 0, 128, 128, 0);
  }
  GemmArgs q_pb(int l) const {
    return gemm_args(w.PL2 + 896, B * NL, 0, 1024, B * NL, LW(l, DD_PB_W2q), LW(l, DD_PB_b2q), LW(l, DD_PB_lnq), w.ql2, B * NL, 0, 128, 128, 0);
  }
  // -- h_out = h + lin_node(A) (+ A_nb on the ligand rows, where the NB sub-layer left it in a buffer of its own)
  GemmArgs lin(int l, float* h, const float* anb) const {
    return add_anb(gemm_args(w.A, B * N, 0, 128, B * N, LW(l, DD_W_lin), LW(l, DD_b_lin), nullptr, h, B * N, 0, 128, 128, 1), anb, true);
  }
  // -- heads, first Linear (decompdiff.py:194-211): bond head on h_bond, v head on the ligand rows of h; pre_att bond head:
  //    P = W_p h of the ligand rows (w.P is free after the node launch)
  GemmArgs bond_head1() const { return gemm_args(w.hb, nE, 0, 128, nE, GW(DD_G_BH_W1), GW(DD_G_BH_b1), nullptr, w.qb, nE, 0, 128, 128, 0); }
  GemmArgs v_head1(const float* h) const {   // (hidden -> qn: ql may still be read by the overlapped coordinate sub-layer)
    return gemm_args(h + (long)NP * 128, NL, hN, 128, B * NL, GW(DD_G_VH_W1), GW(DD_G_VH_b1), nullptr, w.qn, B * NL, 0, 128, 128, 0);
  }
  GemmArgs pre_att_p(const dd_bond_head* bh, const float* h) const {
    return gemm_args(h + (long)NP * 128, NL, hN, 128, B * NL, bh->W_p, nullptr, nullptr, w.P, B * NL, 0, 128, 128, 0);
  }

  // First-Linear projections of layer `l` from h / h_bond (one launch) and the query MLPs' second layer (one launch):
  // the forward's own launches, also run by dd_layer0_tables on its 16-atom problem.
  // (anb != NULL: the previous layer's W_lin . A_nb is still pending on the ligand rows of h -- lin_node inside the node launch)
  int launch_projections1(int l, const float* h, hipStream_t sx, const float* anb = nullptr) const {
    GemmList j;
    j.add(add_anb(n1(l, h), anb, true));
    j.add(add_anb(l1(l, h), anb, false));
    j.add(b1(l));
    return j.launch(sx);
  }
  int launch_queries(int l, bool x2_sum, hipStream_t sx) const {
    GemmList j;
    j.add(q_bl(l, x2_sum));
    j.add(q_ne(l));
    j.add(q_nb(l));
    return j.launch(sx);
  }

  // -- attention sub-layers at layer l, positions x: what every schedule passes; the call sites add what depends on the schedule
  AttnArgs attn_common(const float* x) const {
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.np_real = s->np_real; a.nl_real = s->nl_real;
    a.B = B; a.NP = NP; a.NL = NL; a.K = K; a.x = x;
    return a;
  }
  // node_layer_with_edge (l0_here: this layer's projection / query rows came from the layer-0 tables)
  AttnArgs attn_ne(int l, const float* x, bool l0_here) const {
    AttnArgs ne = attn_common(x);
    ne.nbr = w.nbr; ne.ew = w.ew;
    const float* Pn = l0_here ? s->l0_P : w.P;
    ne.kd = Pn; ne.ks = Pn + 128; ne.vd = Pn + 256; ne.vs = Pn + 384; ne.ld_kd = ne.ld_ks = ne.ld_vd = ne.ld_vs = 640;
    ne.q = l0_here ? s->l0_qn : w.qn; ne.Akp = LW(l, DD_NE_Akp); ne.Avp = LW(l, DD_NE_Avp); ne.lnk = LW(l, DD_NE_lnk); ne.lnv = LW(l, DD_NE_lnv);
    ne.W2k = LW(l, DD_NE_W2k); ne.W2v = LW(l, DD_NE_W2v); ne.b2v = LW(l, DD_NE_b2v); ne.out = w.A;
    // persistent node_layer_with_edge workgroups of the fused launch: two block counters per layer, DD_NUM_COUNTERS holds 32 layers' worth
    ne.work_counter = (l < 32) ? w.counters + 128 + 2 * l : nullptr;
    return ne;
  }
  // node_layer_with_bond: its rows [B * NL, 128] assigned to a buffer of their own
  AttnArgs attn_nb(int l, const float* x) const {
    AttnArgs nb = attn_common(x);
    nb.kd = w.PL; nb.ks = w.PL + 128; nb.vd = w.PL + 256; nb.vs = w.PL + 384; nb.ld_kd = nb.ld_ks = nb.ld_vd = nb.ld_vs = 1280;
    nb.ke = w.PB; nb.ve = w.PB + 128; nb.ld_ke = nb.ld_ve = 640;
    nb.q = w.qlnb; nb.lnk = LW(l, DD_NB_lnk); nb.lnv = LW(l, DD_NB_lnv);
    nb.W2k = LW(l, DD_NB_W2k); nb.W2v = LW(l, DD_NB_W2v); nb.b2v = LW(l, DD_NB_b2v); nb.out = w.Anb; nb.out_assign = 1;
    return nb;
  }
  // bond_layer (residual add into h_bond)
  AttnArgs attn_bl(int l, const float* x) const {
    AttnArgs bl = attn_common(x);
    bl.bl_prefix = s->bl_prefix;
    bl.ke = w.Ek; bl.ve = w.Ev; bl.ld_ke = bl.ld_ve = 128;
    bl.q = w.qb; bl.Wakp = LW(l, DD_BL_Wakp); bl.Wavp = LW(l, DD_BL_Wavp);
    bl.lnk = LW(l, DD_BL_lnk); bl.lnv = LW(l, DD_BL_lnv);
    bl.W2k = LW(l, DD_BL_W2k); bl.W2v = LW(l, DD_BL_W2v); bl.b2v = LW(l, DD_BL_b2v); bl.out = w.hb;
    bl.Rk = w.Rk; bl.Rv = w.Rv;
    bl.work_counter = w.counters + l;                    // persistent workgroups; [0, 64) of the counters: num_blocks * num_layers <= 64
    return bl;
  }
  // pos_layer_with_edge / pos_layer_with_bond
  AttnArgs attn_pe(int l, const float* x) const {
    AttnArgs pe = attn_common(x);
    pe.nbr = w.nbr; pe.ew = w.ew;
    pe.kd = w.PL2; pe.vd = w.PL2 + 128; pe.ld_kd = pe.ld_vd = 1024; pe.ks = w.P2; pe.vs = w.P2 + 128; pe.ld_ks = pe.ld_vs = 256;
    pe.q = w.ql; pe.Akp = LW(l, DD_PE_Akp); pe.Avp = LW(l, DD_PE_Avp); pe.lnk = LW(l, DD_PE_lnk); pe.lnv = LW(l, DD_PE_lnv);
    pe.W2k = LW(l, DD_PE_W2k); pe.W2v16 = LW(l, DD_PE_W2v); pe.b2v16 = LW(l, DD_PE_b2v); pe.out = w.dxe;
    return pe;
  }
  AttnArgs attn_pb(int l, const float* x) const {
    AttnArgs pb = attn_common(x);
    pb.kd = w.PL2 + 384; pb.ks = w.PL2 + 512; pb.vd = w.PL2 + 640; pb.vs = w.PL2 + 768; pb.ld_kd = pb.ld_ks = pb.ld_vd = pb.ld_vs = 1024;
    pb.ke = w.PB2; pb.ve = w.PB2 + 128; pb.ld_ke = pb.ld_ve = 256;
    pb.q = w.ql2; pb.lnk = LW(l, DD_PB_lnk); pb.lnv = LW(l, DD_PB_lnv);
    pb.W2k = LW(l, DD_PB_W2k); pb.W2v16 = LW(l, DD_PB_W2v); pb.b2v16 = LW(l, DD_PB_b2v); pb.out = w.dxb;
    return pb;
  }
  // q_in_pos: the coordinate launch evaluates the second layer of its query MLPs itself (q_pe / q_pb are then not launched)
  void set_q_in_pos(int l, AttnArgs& pe, AttnArgs& pb) const {
    pe.qhid = w.PL2 + 256; pe.ld_qhid = 1024; pe.lnq = LW(l, DD_PE_lnq); pe.W2q = LW(l, DD_PE_W2qT); pe.b2q = LW(l, DD_PE_b2q);
    pb.qhid = w.PL2 + 896; pb.ld_qhid = 1024; pb.lnq = LW(l, DD_PB_lnq); pb.W2q = LW(l, DD_PB_W2qT); pb.b2q = LW(l, DD_PB_b2q);
  }

  // -- head of a forward and block boundaries (dd_graph.hip)
  // kNN graph + edge weights into w.nbr / w.ew: of x_t where the step kernels left it (the sampler's position buffers) ...
  GraphArgs graph_head() const {
    GraphArgs g{};
    g.B = B; g.NP = NP; g.NL = NL; g.K = K;
    g.prot = s->protein_pos; g.prot_stride = 3 * NP; g.lig = s->lig_pos; g.lig_stride = 3 * NL;
    g.nbr = w.nbr; g.ew = w.ew;
    g.EW_W1T = GW(DD_G_EW_W1T); g.EW_b1 = GW(DD_G_EW_b1); g.EW_ln = GW(DD_G_EW_ln); g.EW_w2 = GW(DD_G_EW_w2); g.EW_b2 = GW(DD_G_EW_b2);
    g.np_real = s->np_real; g.nl_real = s->nl_real;
    return g;
  }
  // ... or of one [B, N, 3] block x: the current coordinates at a block boundary (num_blocks > 1), the workspace copy of x_t
  GraphArgs graph_at(const float* x) const {
    GraphArgs g = graph_head();
    g.set_block(x);
    return g;
  }
  // embeddings / context / zeroed counters (advance != NULL: the launch advances the step counter too)
  EmbedArgs embed(int32_t* advance) const {
    EmbedArgs e{};
    e.B = B; e.NP = NP; e.NL = NL; e.nv = num_v(s);
    e.protein_h = s->protein_h; e.protein_pos = s->protein_pos; e.lig_pos = s->lig_pos; e.lig_v = s->lig_v; e.lig_aux = s->lig_aux;
    e.bond = s->lig_bond;
    e.Wl = GW(DD_G_W_lemb); e.bl = GW(DD_G_b_lemb); e.Wb = GW(DD_G_W_bemb); e.bb = GW(DD_G_b_bemb);
    e.h = w.h; e.xa = w.xa; e.xb = w.xb; e.hb = w.hb;
    e.counters = w.counters; e.advance = advance;
    e.bond_rows = (long)B * Eb;
    e.node_blocks = (int)(((long)B * N * 128 + 255) / 256);
    e.blocks = e.node_blocks + (int)((e.bond_rows * 128 + 255) / 256);
    return e;
  }
  // the first layer's projection / query rows of the ligand atoms and bonds gathered from s->l0_tables
  Layer0RowsArgs l0_rows() const {
    Layer0RowsArgs r{};
    r.B = B; r.NP = NP; r.NL = NL;
    r.tab = s->l0_tables; r.lig_v = s->lig_v; r.lig_aux = s->lig_aux; r.bond = s->lig_bond;
    r.l0_P = s->l0_P; r.PL = w.PL; r.l0_qn = s->l0_qn; r.qlnb = w.qlnb; r.PB = w.PB; r.qb = w.qb;
    r.pl_width = plw;
    r.atom_f4 = (long)B * NL * l0_atom_f4(plw);
    r.blocks = (int)((r.atom_f4 + (long)B * Eb * DD_L0_BOND_F4 + 255) / 256);
    return r;
  }
  // the two in one launch (l0: with the layer-0 rows)
  int launch_head_rows(bool l0, int32_t* advance, hipStream_t sx) const {
    const Layer0RowsArgs r = l0_rows();
    return dd::launch_head_rows(embed(advance), l0 ? &r : nullptr, sx);
  }
  // bond-layer assemble of layer l at positions x (q1 NULL: the query GEMM sums its hidden rows itself); the call sites add a
  // deferred coordinate update (xprev / xout; its addends are w.dxe / w.dxb) and the tile-queue wait
  AssembleArgs assemble(int l, const float* x, float* q1) const {
    AssembleArgs a{};
    a.x = x; a.PB = w.PB; a.PL = w.PL; a.Wgp = LW(l, DD_BL_Wgp);
    a.B = B; a.NP = NP; a.NL = NL;
    a.narrow = narrow;
    a.Ek = w.Ek; a.Ev = w.Ev; a.q1 = narrow ? nullptr : q1; a.Rk = w.Rk; a.Rv = w.Rv;
    a.dxe = w.dxe; a.dxb = w.dxb;
    a.fw = no_wait();
    return a;
  }
};

#if defined(DD_DEBUG_OPTIONS) && DD_DEBUG_OPTIONS
// ---------------------------------------------------------------------------------------------------------------------
// Schedule 5 (measurement build only; EXPERIMENTS.md, round 3): the dense GEMMs between two node attentions as TWO ordered
// tile queues per layer (dd_gemm.hip::k_gemm_tail: tickets in dependency order, write-through tiles, device counters) --
// `ta` = lin_node + the coordinate sub-layers' projections on the main stream in front of the coordinate attention, `tb`
// = the next layer's projections and query MLPs (last layer: the heads' first Linear) on the side stream -- and device
// counters instead of graph edges towards the next assemble / node attention (they poll; the side stream is joined once
// per forward).  Bit-identical to schedule 4, 31 instead of 51 launches per step, and SLOWER (1.41 vs 1.24 ms/step): a
// polling consumer with a large per-CU footprint keeps the producers' workgroups off the chip.  `two_streams` false
// (profiling): the same launches on one stream -- every wait is then satisfied when it is reached.
static int forward_tail(const Fwd& f, DevCtx& dc, hipStream_t st, StepFold* fold, bool two_streams) {
  const dd_sampler* s = f.s;
  const Workspace& w = f.w;
  const int B = f.B, NP = f.NP, NL = f.NL, N = f.N, nE = f.nE, L = s->num_layers;
  int32_t* flags = w.counters + DD_NUM_COUNTERS;
  auto FL = [&](int l, int fl) { return (l * DD_FLAGS_PER_LAYER + fl) * DD_FLAG_STRIDE; };
  if (two_streams) DD_TRY(ensure_side_stream(dc));
  const bool l0 = g_l0_tables && s->l0_tables && s->l0_P && s->l0_qn && s->nl_real == nullptr;
  int32_t* advance = (fold && fold->advance) ? s->step_counter : nullptr;

  // ---- head of the forward: kNN graph + edge weights (side stream) beside embeddings / context / zeroed counters and
  //      flags / layer-0 rows (main stream); decompdiff.py:219-297, uni_transformer_edge.py:404-427
  bool head_join = false;
  if (two_streams) {
    if (hipEventRecord(dc.ev_fork[8], st) != hipSuccess || hipStreamWaitEvent(dc.side, dc.ev_fork[8], 0) != hipSuccess) return DD_ERR_HIP;
    DD_TRY(launch_graph(f.graph_head(), dc.side));
    if (hipEventRecord(dc.ev_join[8], dc.side) != hipSuccess) return DD_ERR_HIP;
    head_join = true;
    DD_TRY(f.launch_head_rows(l0, advance, st));
  } else {
    DD_TRYP(DD_PROF_MISC, f.launch_head_rows(l0, advance, st));
    DD_TRYP(DD_PROF_MISC, launch_graph(f.graph_head(), st));
  }
  if (!l0) {                                             // first layer's projections / queries as GEMMs (no tables)
    DD_TRYP(DD_PROF_GEMM, f.launch_projections1(0, w.h, st));
    DD_TRYP(DD_PROF_GEMM, f.launch_queries(0, true, st));
  }
  // tile counts of the queue's jobs (targets of the counters)
  const int n_lin = gemm_tiles(B * N, 128), n_p2 = gemm_tiles(B * N, 256), n_pl2 = gemm_tiles(B * NL, 1024), n_pb2 = gemm_tiles(nE, 256);
  const int n_pl1 = gemm_tiles(B * NL, 1280), n_p1q = gemm_tiles(B * N, 128), n_p1r = gemm_tiles(B * N, 512);
  const int n_pbq = gemm_tiles(nE, 128), n_pb1r = gemm_tiles(nE, 512);
  const int n_q = gemm_tiles(B * N, 128) + gemm_tiles(B * NL, 128) + gemm_tiles(nE, 128);
  const int total_mid = n_lin + n_p2 + n_pl2 + n_pb2 + n_pl1 + n_p1q + n_p1r + n_pbq + n_pb1r + n_q;

  float* xcur = w.xa;
  float* xnext = w.xb;
  const float* xup_prev = nullptr;
  for (int l = 0; l < L; ++l) {
    // ---- assemble (bond_layer first-Linear partial sums; applies the previous layer's coordinate update)
    FlagWait fw = no_wait();
    if (l > 0) fw = FlagWait{flags, FL(l - 1, DD_FLAG_PB1R), n_pb1r, FL(l - 1, DD_FLAG_PL1), n_pl1};
    AssembleArgs as = f.assemble(l, xcur, nullptr);
    as.xprev = xup_prev; as.xout = xup_prev ? xcur : nullptr; as.fw = fw;
    DD_TRYP(DD_PROF_ASSEMBLE, launch_bl_assemble(as, st));
    xup_prev = nullptr;
    if (head_join) {                                     // kNN graph + edge weights: first needed by the node attention
      if (hipStreamWaitEvent(st, dc.ev_join[8], 0) != hipSuccess) return DD_ERR_HIP;
      head_join = false;
    }
    // ---- node_layer_with_edge + node_layer_with_bond + bond_layer: one launch (uni_transformer_edge.py:42-167)
    {
      AttnArgs ne = f.attn_ne(l, xcur, l0 && l == 0);
      if (l > 0) {                                       // (its other inputs -- PB, PL -- were awaited by this layer's assemble)
        ne.wait_flags = flags; ne.wait_idx = FL(l - 1, DD_FLAG_NODE); ne.wait_n = n_q + n_p1r;
      }
      DD_TRYP(DD_PROF_ATTN_BL, launch_attn2_node(ne, f.attn_nb(l, xcur), f.attn_bl(l, xcur), st));
    }
    // ---- the two tile queues of the layer: `ta` (lin_node + the coordinate sub-layers' projections: what the coordinate
    //      attention needs) on the main stream, `tb` (next layer's projections / queries, or the heads) on the side stream
    TailArgs ta, tb;
    {
      memset(&ta, 0, sizeof(ta));
      memset(&tb, 0, sizeof(tb));
      ta.flags = tb.flags = flags;
      ta.ticket = FL(l, DD_FLAG_TICKET);
      tb.ticket = FL(l, DD_FLAG_TICKET2);
      const int fLIN = FL(l, DD_FLAG_LIN), fNODE = FL(l, DD_FLAG_NODE);
      const int fPOS = -1;                               // (the coordinate launch follows `ta` in stream order)
      int n = 0;
      ta.job[n++] = tail_job(f.lin(l, w.h, w.Anb), -1, 0, fLIN);                        // h += lin_node(A + A_nb on ligand rows)
      // (independent tiles right behind lin_node: the workgroups of the first wave work instead of polling for it)
      ta.job[n++] = tail_job(f.b2(l), -1, 0, fPOS);
      ta.job[n++] = tail_job(f.n2(l, w.h), fLIN, n_lin, fPOS);
      ta.job[n++] = tail_job(f.l2(l, w.h), fLIN, n_lin, fPOS);
      ta.njobs = n;
      n = 0;
      if (l + 1 < L) {
        const int ll = l + 1;
        const int fPL1 = FL(l, DD_FLAG_PL1), fP1Q = FL(l, DD_FLAG_P1Q), fPBQ = FL(l, DD_FLAG_PBQ), fPB1R = FL(l, DD_FLAG_PB1R);
        // next layer's projections: the query-hidden column blocks first (their consumers sit at the end of the list)
        tb.job[n++] = tail_job(f.b1(ll, 512, 128), -1, 0, fPBQ);
        tb.job[n++] = tail_job(f.l1(ll, w.h), fLIN, n_lin, fPL1);
        tb.job[n++] = tail_job(f.n1(ll, w.h, 512, 128), fLIN, n_lin, fP1Q);
        tb.job[n++] = tail_job(f.b1(ll, 0, 512), -1, 0, fPB1R);
        tb.job[n++] = tail_job(f.n1(ll, w.h, 0, 512), fLIN, n_lin, fNODE);
        // next layer's query MLPs, second Linear (LayerNorm + ReLU prologue); the bond-layer hidden row is
        // q_hb[bond] + q_hi[destination atom], summed while the tile stages its rows
        tb.job[n++] = tail_job(f.q_ne(ll), fP1Q, n_p1q, fNODE);
        tb.job[n++] = tail_job(f.q_nb(ll), fPL1, n_pl1, fNODE);
        tb.job[n++] = tail_job(f.q_bl(ll, true), fPBQ, n_pbq, fNODE, fPL1, n_pl1);
      } else {
        // heads, first Linear: bond head on h_bond, v head on the ligand rows of the new h
        tb.job[n++] = tail_job(f.bond_head1(), -1, 0, fNODE);
        tb.job[n++] = tail_job(f.v_head1(w.h), fLIN, n_lin, fNODE);
      }
      tb.njobs = n;
    }
    // ---- pos_layer_with_edge + pos_layer_with_bond: one launch (uni_transformer_edge.py:188-210), query MLPs inside
    {
      AttnArgs pe = f.attn_pe(l, xcur), pb = f.attn_pb(l, xcur);
      f.set_q_in_pos(l, pe, pb);
      if (two_streams) {
        // Recording order matters: the graph runtime keeps the FIRST-recorded successor of a node on that node's hardware
        // queue and pays the cross-queue latency (7-12 us) on the others -- `ta`, which gates the coordinate attention,
        // is recorded first; `tb` has ~50 us of slack before its first consumer (the next assemble) polls its counters.
        if (hipEventRecord(dc.ev_fork[l], st) != hipSuccess) return DD_ERR_HIP;
        DD_TRY(launch_gemm_tail(ta, st));
        if (hipStreamWaitEvent(dc.side, dc.ev_fork[l], 0) != hipSuccess) return DD_ERR_HIP;
        DD_TRY(launch_gemm_tail(tb, dc.side));
        if (l + 1 == L && hipEventRecord(dc.ev_join[l], dc.side) != hipSuccess) return DD_ERR_HIP;
        DD_TRY(launch_attn2_pos(pe, pb, st));
      } else {
        DD_TRYP(DD_PROF_GEMM, launch_gemm_tail(ta, st));
        DD_TRYP(DD_PROF_GEMM, launch_gemm_tail(tb, st));
        DD_TRYP(DD_PROF_ATTN_PE, launch_attn2_pos(pe, pb, st));
      }
      if (l + 1 < L && ta.total + tb.total != total_mid) return DD_ERR_BAD_ARG;       // (the counters' targets follow the job lists)
      // x += dx_edge + dx_bond (ligand rows, :285) is applied by the next consumer of x: the next layer's assemble launch,
      // or the step kernel behind the last layer (folded step boundary); a plain forward runs the 3-block update launch
      const bool deferred = l + 1 < L || (fold && fold->fold_tail);
      if (deferred) xup_prev = xcur;
      else DD_TRYP(DD_PROF_MISC, launch_xupdate(xcur, w.dxe, w.dxb, B, NP, NL, xnext, st));
    }
    float* t = xcur; xcur = xnext; xnext = t;
  }
  if (head_join && hipStreamWaitEvent(st, dc.ev_join[8], 0) != hipSuccess) return DD_ERR_HIP;
  if (two_streams && hipStreamWaitEvent(st, dc.ev_join[L - 1], 0) != hipSuccess) return DD_ERR_HIP;   // last queue: the heads' hidden rows
  if (!s->pred_pos) return DD_ERR_BAD_ARG;
  if (xup_prev != nullptr) {                             // folded tail: the step kernel applies the update and extracts x0
    fold->xprev = xup_prev;
    return DD_OK;
  }
  DD_TRYP(DD_PROF_MISC, launch_extract_ligand(xcur, B, NP, NL, s->pred_pos, st));
  return DD_OK;
}

#endif

// Node output MLPs (x2h_out_fc; include/decompdiff_hip.h dd_node_out): NULL = a model without them
static int check_node_out(const dd_node_out* no, const dd_sampler* s) {
  if (no == nullptr) return DD_OK;
  if (!s || no->num_layers != s->num_layers || no->num_layers < 1 || no->num_layers > 64) return DD_ERR_BAD_ARG;
  for (int l = 0; l < no->num_layers; ++l)
    if (!no->layer[l] || (reinterpret_cast<size_t>(no->layer[l]) & 15) != 0) return DD_ERR_BAD_ARG;
  return DD_OK;
}

// What the model is beyond the dd_sampler: the contents of a dd_model_opts (include/decompdiff_hip.h), checked.
struct ModelOpts {
  const dd_bond_head* bh = nullptr;
  const dd_node_out* no = nullptr;
  int num_blocks = 1;
};
// What a chain's reverse steps take beyond the model: the arguments of the *_keyed / *_fixed / *_resample / *_guided entry points,
// checked and held by value (read_step_extras)
struct StepExtras {
  const uint64_t* sample_keys = nullptr;   // per-sample noise keys ([B], device, read at every launch) or NULL
  bool has_fixed = false;
  dd_fixed fixed = {};                     // has_fixed: the fixed atoms (device pointers, read at every launch)
  const int32_t* epoch = nullptr;          // resampling epoch (a device int, read at every launch) or NULL
  bool has_restraints = false;
  RestraintArgs restraints = {};           // has_restraints: the distance restraints
};
static int check_blocks(const dd_sampler* s, int num_blocks) {
  if (!s || num_blocks < 1) return DD_ERR_BAD_ARG;
  // every step of a forward has a bond-layer work counter of its own (Workspace::counters [0, 64))
  return (long)num_blocks * s->num_layers <= 64 ? DD_OK : DD_ERR_UNSUPPORTED_SHAPE;
}

// The score network: num_blocks * num_layers steps; step l runs layer l % num_layers (shared weights), and every step with
// l % num_layers == 0, l > 0 opens a new block: its kNN graph and edge weights are rebuilt from the coordinates the previous
// block left (uni_transformer_edge.py:402-437).  Everything that ping-pongs by layer parity (x, A / Anb) and every per-layer
// counter goes by the step, so one block is exactly the former loop.
static int forward_impl(const dd_sampler* s, hipStream_t st, StepFold* fold = nullptr, const ModelOpts& mo = ModelOpts()) {
  const dd_bond_head* bh = mo.bh;
  const dd_node_out* no = mo.no;
  DD_TRY(check_shapes(s));
  DD_TRY(check_node_out(no, s));
  DD_TRY(check_blocks(s, mo.num_blocks));
  const bool pre_att = is_pre_att(bh);
  // x2h_out_fc: k_node_out_fc (node output MLPs + lin_node, one launch) takes the place of the lin_node GEMM job; the node
  // launch's in-kernel lin_node has no node-output stage, so lin_in_node is off for such a model
  const bool out_fc = no != nullptr;
  const Fwd f(s);
  const Workspace& w = f.w;
  const int B = f.B, NP = f.NP, NL = f.NL, N = f.N;
  const int LB = s->num_layers, L = mo.num_blocks * LB;  // layers of a block; steps of the forward
  DevCtx& dc = dev_ctx();                                // side stream + fork / join events of this device

  float* xcur = w.xa;
  float* xnext = w.xb;
  float* hcur = w.h;                                     // (ping-pong with w.h2 under the one-fork schedule only)
  const bool fused = g_fuse && NL <= g_fused_max_nl && g_dbg_clock == nullptr;
  // (the per-layer fork / join events are taken round robin, slot step & 7: an event is waited for at most one step after it
  //  was recorded, and recording it again later -- eager or while capturing -- makes a new dependency)
  const bool overlap = fused && g_overlap && g_prof == nullptr && LB <= 8;
  auto ev = [](int l) { return l & 7; };
#if defined(DD_DEBUG_OPTIONS) && DD_DEBUG_OPTIONS
  if (out_fc && (g_sched >= 5 || g_side_lin)) return DD_ERR_UNSUPPORTED_SHAPE;   // (measurement schedules without the node-output stage)
  if (mo.num_blocks > 1 && (g_sched >= 5 || g_side_lin)) return DD_ERR_UNSUPPORTED_SHAPE;   // (... and without the block boundary)
  if (fused && !pre_att && !f.narrow && g_sched >= 5 && L <= DD_FLAG_LAYERS && g_q1_in_gemm && g_gemm_ksplit_on() && g_q_in_pos && g_head_fused &&
      g_xup_in_asm && !g_xup_in_pos)
    return forward_tail(f, dc, st, fold, overlap);
#endif
  if (out_fc && !fused) return DD_ERR_UNSUPPORTED_SHAPE;   // (the one-launch-per-sub-layer loop has no node-output stage)
  if (overlap) DD_TRY(ensure_side_stream(dc));

  // layer-0 tables: the first layer's projection and query rows are gathered (ligand atoms: 16 combinations of class and
  // arm flag, bonds: type x destination combination; protein rows are static per chain) instead of two GEMM launches
  const bool l0 = fused && g_l0_tables && g_q1_in_gemm && g_gemm_ksplit_on() && s->l0_tables && s->l0_P && s->l0_qn &&
                  s->nl_real == nullptr;
  int32_t* advance = (fold && fold->advance) ? s->step_counter : nullptr;
  bool head_join = false;
  if (overlap && g_head_fused) {
    // dd_graph.hip: the graph (k_graph: kNN + edge weights, one wave per centre, reading x_t from the sampler's
    // position buffers) forked to the side stream FIRST, the embeddings / context / counters / layer-0 rows (k_head_rows)
    // on the main stream beside it -- two launches instead of four.  (Measured and dropped: all four bodies in one
    // kernel, +2.5 % step time -- one register allocation for every block kind, and assemble then waits for a graph it
    // does not need; rows first and the graph forked after them, +1 %.)
    if (hipEventRecord(dc.ev_fork[8], st) != hipSuccess || hipStreamWaitEvent(dc.side, dc.ev_fork[8], 0) != hipSuccess) return DD_ERR_HIP;
    // (option 29: the rows launch is RECORDED first -- same dependencies, the fork point is the event above -- so that the graph
    // runtime, which keeps the first-recorded successor of a node on its hardware queue, leaves the main chain's launch on the
    // previous step kernel's queue and moves the graph construction, which has slack, to the other one)
    if (g_head_rows_first) DD_TRYP(DD_PROF_MISC, f.launch_head_rows(l0, advance, st));
    DD_TRYP(DD_PROF_MISC, launch_graph(f.graph_head(), dc.side));
    if (hipEventRecord(dc.ev_join[8], dc.side) != hipSuccess) return DD_ERR_HIP;
    head_join = true;
    if (!g_head_rows_first) DD_TRYP(DD_PROF_MISC, f.launch_head_rows(l0, advance, st));
  } else {
    // embeddings + context (decompdiff.py:219-297) and the zeroed work counters: one launch
    DD_TRYP(DD_PROF_MISC, launch_embed(f.embed(advance), st));
    if (l0) DD_TRYP(DD_PROF_MISC, launch_layer0_rows(f.l0_rows(), st));
    // graph (uni_transformer_edge.py:404-427): only the attention kernels need it, so with two streams it is built
    // beside the bond embedding and the first layer's projections
    hipStream_t gs = st;
    if (overlap) {
      if (hipEventRecord(dc.ev_fork[8], st) != hipSuccess || hipStreamWaitEvent(dc.side, dc.ev_fork[8], 0) != hipSuccess) return DD_ERR_HIP;
      gs = dc.side;
    }
    const GraphArgs g = f.graph_at(w.xa);                // (the workspace copy of x_t the embedding launch just wrote)
    DD_TRYP(DD_PROF_MISC, launch_knn(g, gs));
    DD_TRYP(DD_PROF_MISC, launch_edge_weights(g, gs));
    if (overlap) {
      if (hipEventRecord(dc.ev_join[8], dc.side) != hipSuccess) return DD_ERR_HIP;
      head_join = true;
    }
  }
  int pending_join = -1;
  bool heads_done = false;
  // lin_node inside the node launch (g_lin_in_node): the NE blocks update h in place, the NB blocks leave W_lin . A_nb of layer l
  // in anb_buf(l) (ping-pong between w.Anb and w.A, which no longer holds the attention output); every consumer of the new h
  // adds it to the ligand rows (GemmArgs::X2, Fwd::add_anb) and the next layer's NE blocks fold it into h
  const bool lin_in_node = uses_lin_in_node(B, NL, out_fc, fused);
  // (schedule 0) the coordinate launch of layer l is *recorded* after the next layer's projection / query GEMMs: the graph
  // runtime keeps the first-recorded successor of a node on the same hardware queue, and the branch that pays the
  // 10-12 us of cross-queue fork + join latency must be the short one (coordinates), not the GEMM chain
  struct DeferredPos { bool armed; AttnArgs pe, pb; float *xcur, *xnext; int layer; bool xup; } dpos;
  dpos.armed = false;
  auto flush_pos = [&]() -> int {
    if (!dpos.armed) return DD_OK;
    dpos.armed = false;
    if (hipStreamWaitEvent(dc.side, dc.ev_fork[ev(dpos.layer)], 0) != hipSuccess) return DD_ERR_HIP;
    int rc = launch_attn2_pos(dpos.pe, dpos.pb, dc.side);
    if (rc == DD_OK && !dpos.xup) rc = launch_xupdate(dpos.xcur, w.dxe, w.dxb, B, NP, NL, dpos.xnext, dc.side);
    if (rc != DD_OK) return rc;
    if (hipEventRecord(dc.ev_join[ev(dpos.layer)], dc.side) != hipSuccess) return DD_ERR_HIP;
    pending_join = ev(dpos.layer);
    return DD_OK;
  };
  const float* xup_prev = nullptr;                       // != nullptr: x of the previous layer, its update still pending
  for (int l = 0; l < L && fused; ++l) {
    const bool last = l + 1 == L;
    // ---- projections of the old h / h_bond: one launch (the q blocks are the last columns: skipped when fused above).
    //      With the projection-ahead schedule this launch was already issued on the side stream right after the
    //      previous layer's lin_node (it needs h and h_bond only) and is joined before its first consumer.
    // (W_lin . A_nb pending on the ligand rows of h: the previous layer's at the head of this layer, this layer's behind the node launch)
    const float* const anb_prev = (lin_in_node && l > 0) ? f.anb_buf(l - 1) : nullptr;
    const float* const anb_new = lin_in_node ? f.anb_buf(l) : nullptr;
    // (called for THIS layer at its head or for the NEXT one behind the node launch)
    auto launch_batch1 = [&](int ll, hipStream_t sx) -> int { return f.launch_projections1(ll, hcur, sx, ll == l ? anb_prev : anb_new); };
    // (schedule 2) the same projections in two launches: the bond part only needs h_bond, final once the node
    // attention is done; the node parts (called for the NEXT layer) need h (lin_node)
    // (hsrc: the h the node parts read; lin_dup: the lin_node job that forms it first, one-fork schedule)
    auto launch_batch1_part = [&](int ll, int part, hipStream_t sx, const float* hsrc, const GemmArgs* lin_dup) -> int {
      GemmList j;
      if (part == 0) {
        if (lin_dup) j.add(*lin_dup);                      // (the small job first: its consumers are the next launch)
        j.add(f.b1(ll));
      } else {
        j.add(f.add_anb(f.n1(ll, hsrc), anb_new, true));
        j.add(f.add_anb(f.l1(ll, hsrc), anb_new, false));
      }
      return j.launch(sx);
    };
    const bool ahead = overlap && g_sched >= 1;
    const bool ahead_split = overlap && g_sched >= 2;
    const bool ahead_b2 = overlap && g_sched >= 3 && g_q1_in_gemm && g_gemm_ksplit_on();
    const bool two_joins = ahead_b2 && g_sched >= 4;     // ev_qb_fork[l]: layer l's projections done (side stream)
    const bool proj_main = lin_in_node && g_lin_proj_main && two_joins && ahead_split;   // next layer's node projections in the main launch
    const bool pb_early = g_pb_early && g_lin_with_pb2 && !ahead && !lin_in_node;   // next layer's bond projections ride with lin_node
    const bool l0_here = l0 && l == 0;                  // this layer's projection / query rows came from the tables
    if (pb_early && l > 0) DD_TRYP(DD_PROF_GEMM, launch_batch1_part(l, 1, st, hcur, nullptr));
    else if (!(ahead && l > 0) && !l0_here) DD_TRYP(DD_PROF_GEMM, launch_batch1(l, st));
    // ---- queries (second Linear of the q MLPs, LayerNorm+ReLU prologue): one launch.  The bond-layer hidden row is
    //      q_hb[bond] + q_hi[dst atom], summed while the GEMM stages its rows, so this launch depends on the projections
    //      only and runs before the coordinates of the previous layer are joined.
    const bool q1_in_gemm = g_q1_in_gemm && g_gemm_ksplit_on();
    auto launch_b2 = [&](int ll, hipStream_t sx) -> int { return f.launch_queries(ll, q1_in_gemm, sx); };
    // (schedule 3) the query GEMMs of this layer already ran on the side stream behind its projections
    const bool b2_ahead = ahead_b2 && q1_in_gemm && l > 0;
    bool b1_joined = false;
    if (q1_in_gemm && !b2_ahead) {
      if (ahead && l > 0) {                              // (schedules 1/2: this layer's projections ran on the side stream)
        if (hipStreamWaitEvent(st, dc.ev_join[ev(l)], 0) != hipSuccess) return DD_ERR_HIP;
        b1_joined = true;
      }
      if (!l0_here) DD_TRYP(DD_PROF_GEMM, launch_b2(l, st));
    }
    DD_TRY(flush_pos());                                 // previous layer's coordinate launch (side stream)
    if (pending_join >= 0) {
      if (hipStreamWaitEvent(st, dc.ev_join[pending_join], 0) != hipSuccess) return DD_ERR_HIP;
      pending_join = -1;
    }
    const bool late_join = two_joins && b2_ahead && !b1_joined;
    if (ahead && l > 0 && !b1_joined && hipStreamWaitEvent(st, late_join ? dc.ev_qb_fork[ev(l)] : dc.ev_join[ev(l)], 0) != hipSuccess)
      return DD_ERR_HIP;                                 // projections of this layer
    // (a deferred coordinate update of the previous layer is applied here: xcur's ligand rows are written by this launch)
    AssembleArgs as = f.assemble(l, xcur, q1_in_gemm ? nullptr : w.q1bl);
    as.xprev = xup_prev; as.xout = xup_prev ? xcur : nullptr;
    DD_TRYP(DD_PROF_ASSEMBLE, launch_bl_assemble(as, st));
    xup_prev = nullptr;
    // ---- block boundary: the new block's kNN graph + edge weights from x as the previous block left it.  xcur is complete here
    //      by construction: the previous layer's coordinate launch was flushed and joined above, and its update is applied by
    //      the assemble launch in front of this one (or was, by a launch of its own, on this stream or behind that join).  The
    //      readers of the old graph (previous node launch, previous coordinate launch) are ordered before this launch the same
    //      way; the next ones (this step's node launch, its coordinate launch behind a fork recorded after it) follow it.
    if (l > 0 && l % LB == 0) DD_TRYP(DD_PROF_MISC, launch_graph(f.graph_at(xcur), st));
    if (!q1_in_gemm) DD_TRYP(DD_PROF_GEMM, launch_b2(l, st));
    if (head_join) {                                     // kNN graph + edge weights: first needed by the node attention
      if (hipStreamWaitEvent(st, dc.ev_join[8], 0) != hipSuccess) return DD_ERR_HIP;
      head_join = false;
    }
    if (late_join && hipStreamWaitEvent(st, dc.ev_join[ev(l)], 0) != hipSuccess) return DD_ERR_HIP;   // this layer's query GEMMs
    // ---- node_layer_with_edge + node_layer_with_bond + bond_layer: one launch
    {
      AttnArgs ne = f.attn_ne(l, xcur, l0_here), nb = f.attn_nb(l, xcur);
      if (lin_in_node) {
        ne.out = hcur; ne.lin_W = f.LW(l, DD_W_lin); ne.lin_b = f.LW(l, DD_b_lin); ne.lin_add = anb_prev;
        nb.out = f.anb_buf(l); nb.lin_W = f.LW(l, DD_W_lin);
      }
      DD_TRYP(DD_PROF_ATTN_BL, launch_attn2_node(ne, nb, f.attn_bl(l, xcur), st));
    }
    if (ahead_split && !last && hipEventRecord(dc.ev_qa_fork[ev(l + 1)], st) != hipSuccess) return DD_ERR_HIP;   // h_bond final
    // ---- h += lin_node(A + A_nb on ligand rows)
    // One-fork schedule: the new h goes to the ping-pong partner (h_new = h_old + ...), because the side stream forms the same
    // rows from h_old at the same time (side_lin job below: identical arithmetic, its own output buffer) -- the main stream's
    // lin_node launch then has no successor on the other queue (every such edge costs the main chain ~5 us, EXPERIMENTS.md R3-2)
    const bool side_lin = g_side_lin && ahead_split && ahead_b2 && !last;
    float* const hold = hcur;
    GemmArgs lin_dup;
    if (out_fc) {
      // the jobs that ride with the lin_node GEMM (PB2, next layer's PB) ride with the projections behind this launch instead
      NodeOutArgs na{w.A, w.Anb, hcur, hcur, no->layer[l % LB], B, NP, NL};
      DD_TRYP(DD_PROF_GEMM, launch_node_out_fc(na, st));
    } else if (!lin_in_node) {
      GemmArgs g = f.lin(l, hcur, w.Anb);
      if (side_lin) {
        float* hnew = (hcur == w.h) ? w.h2 : w.h;
        g.Y = hnew; g.acc_src = hold;
        lin_dup = g; lin_dup.Y = w.hs;
        hcur = hnew;
      } else if (hcur != w.h) {                            // last layer after an odd number of moves: the final h lands in w.h
        g.Y = w.h; g.acc_src = hold;                       // (the side stream's last reader of w.h was joined before this layer's
        hcur = w.h;                                        //  node attention)
      }
      if (g_lin_with_pb2) {
        // the bond projections of the coordinate sub-layer only need the new h_bond: they share this launch, so that
        // the launch behind lin_node (projections of the new h) is a third of its former size
        GemmList j;
        j.add(g);
        j.add(f.b2(l));
        if (pb_early && !last) j.add(f.b1(l + 1));         // ... and so do the next layer's bond projections (h_bond is final)
        DD_TRYP(DD_PROF_GEMM, j.launch(st));
      } else {
        DD_TRYP(DD_PROF_GEMM, launch_gemm128(g, st));
      }
    }
    if (ahead && !side_lin && !proj_main && !last && hipEventRecord(dc.ev_fork[ev(l + 1)], st) != hipSuccess) return DD_ERR_HIP;   // h, h_bond final
    // ---- projections of the new h / h_bond: one launch -- {P2, PL2}, and the coordinate sub-layer's bond projections where they
    //      did not ride with the lin_node GEMM.  In the LAST layer the heads' first Linear (decompdiff.py:194-211: bond head on the
    //      final h_bond, v head on the ligand rows of the final h) rides along: it needs nothing the coordinate sub-layers produce,
    //      and as a launch of its own behind them it sat on the step's critical chain (8 us per step).  (lin_in_node: this layer's
    //      W_lin . A_nb is pending on every job that reads the ligand rows of h.)
    GemmList p2;
    p2.add(f.add_anb(f.n2(l, hcur), anb_new, true));
    p2.add(f.add_anb(f.l2(l, hcur), anb_new, false));
    if (!g_lin_with_pb2 || lin_in_node || out_fc) p2.add(f.b2(l));
    if (g_heads_early && g_lin_with_pb2 && last) {
      p2.add(pre_att ? f.add_anb(f.pre_att_p(bh, hcur), anb_new, false) : f.bond_head1());
      p2.add(f.add_anb(f.v_head1(hcur), anb_new, false));
      heads_done = true;
    }
    if (proj_main && !last) {                            // the next layer's node projections (the side stream is the longer branch otherwise)
      p2.add(f.add_anb(f.n1(l + 1, hcur), anb_new, true));
      p2.add(f.add_anb(f.l1(l + 1, hcur), anb_new, false));
    }
    if (out_fc && pb_early && !last) p2.add(f.b1(l + 1));  // (would have shared the lin_node launch)
    // (round 5) these jobs ride INSIDE the coordinate launch below when it can take them (launch_attn2_pos_g): the attention
    // workgroups wait for the first two, the heads' tiles trail behind them
    bool p2_in_pos = g_p2_in_pos && g_lin_with_pb2 && g_q_in_pos && !g_xup_in_pos && g_pos_waves == 4 && NL <= 65 && l < 64 &&
                     !(overlap && !ahead) && !out_fc && !lin_in_node;
    if (!p2_in_pos) DD_TRYP(DD_PROF_GEMM, p2.launch(st));
    if (proj_main && !last && hipEventRecord(dc.ev_fork[ev(l + 1)], st) != hipSuccess) return DD_ERR_HIP;   // P, PL of the next layer
    const bool q_in_pos = g_q_in_pos;           // second layer of the coordinate query MLPs inside attn_pos
    if (!q_in_pos) {
      GemmList j;
      j.add(f.q_pe(l));
      j.add(f.q_pb(l));
      DD_TRYP(DD_PROF_GEMM, j.launch(st));
    }
    // ---- pos_layer_with_edge + pos_layer_with_bond: one launch, then the coordinate update (ligand rows only)
    {
      AttnArgs pe = f.attn_pe(l, xcur), pb = f.attn_pb(l, xcur);
      const bool xup_in_pos = g_xup_in_pos != 0;           // x update by the last workgroup of the coordinate launch
      // ... or by the next layer's assemble launch, the first consumer of the new x (one launch less on the chain)
      const bool xup_in_asm = !xup_in_pos && ((g_xup_in_asm && !last) || (fold && fold->fold_tail && last));   // (... or by the step kernel)
      if (xup_in_pos) { pe.work_counter = w.counters + 32 + (l & 15); pe.x_next = xnext; }
      if (q_in_pos) f.set_q_in_pos(l, pe, pb);
      if (overlap && !ahead) {
        // fork: the coordinate sub-layers run on the side stream and are joined before the next consumer of x
        if (hipEventRecord(dc.ev_fork[ev(l)], st) != hipSuccess) return DD_ERR_HIP;
        dpos.armed = true; dpos.pe = pe; dpos.pb = pb; dpos.xcur = xcur; dpos.xnext = xnext; dpos.layer = l; dpos.xup = xup_in_pos || xup_in_asm;
        if (!g_defer_pos) DD_TRY(flush_pos());
      } else {
        if (p2_in_pos) {
          int rc_g;
          { ProfScope prof_scope__(DD_PROF_ATTN_PE, st); rc_g = launch_attn2_pos_g(pe, pb, p2.j, p2.n, 2, w.counters + 64 + l, st); }
          if (rc_g == DD_ERR_UNSUPPORTED_SHAPE) {          // (e.g. padded output rows): the two launches
            p2_in_pos = false;
            DD_TRYP(DD_PROF_GEMM, p2.launch(st));
          } else if (rc_g != DD_OK) {
            return rc_g;
          }
        }
        if (!p2_in_pos) DD_TRYP(DD_PROF_ATTN_PE, launch_attn2_pos(pe, pb, st));
        if (!xup_in_pos && !xup_in_asm) DD_TRYP(DD_PROF_MISC, launch_xupdate(xcur, w.dxe, w.dxb, B, NP, NL, xnext, st));
      }
      if (xup_in_asm) xup_prev = xcur;
    }
    if (ahead && !last) {                                // (recorded after the main-stream nodes on purpose)
      if (ahead_split) {
        if (hipStreamWaitEvent(dc.side, dc.ev_qa_fork[ev(l + 1)], 0) != hipSuccess) return DD_ERR_HIP;
        DD_TRY(launch_batch1_part(l + 1, 0, dc.side, nullptr, side_lin ? &lin_dup : nullptr));
        if (!side_lin && !lin_in_node && hipStreamWaitEvent(dc.side, dc.ev_fork[ev(l + 1)], 0) != hipSuccess) return DD_ERR_HIP;   // (lin_in_node: h is final with h_bond)
        if (!proj_main) DD_TRY(launch_batch1_part(l + 1, 1, dc.side, side_lin ? w.hs : hcur, nullptr));
        if (two_joins && hipEventRecord(dc.ev_qb_fork[ev(l + 1)], dc.side) != hipSuccess) return DD_ERR_HIP;
        if (proj_main && hipStreamWaitEvent(dc.side, dc.ev_fork[ev(l + 1)], 0) != hipSuccess) return DD_ERR_HIP;   // the main stream's P, PL
        if (ahead_b2) DD_TRY(launch_b2(l + 1, dc.side));
      } else {
        if (hipStreamWaitEvent(dc.side, dc.ev_fork[ev(l + 1)], 0) != hipSuccess) return DD_ERR_HIP;
        DD_TRY(launch_batch1(l + 1, dc.side));
      }
      if (hipEventRecord(dc.ev_join[ev(l + 1)], dc.side) != hipSuccess) return DD_ERR_HIP;
    }
    float* t = xcur; xcur = xnext; xnext = t;
  }
  // One launch per sub-layer (per-kernel timing, the cross-check of the fused launches): the coordinate sub-layers' projections and
  // queries reuse the node sub-layers' buffers, and both NB and PB queries go through w.ql -- the same builders on aliased buffers
  Fwd u = f;
  u.w.P2 = w.P; u.w.PL2 = w.PL; u.w.PB2 = w.PB; u.w.qlnb = u.w.ql2 = w.ql;
  for (int l = 0; l < L && !fused; ++l) {
    if (l > 0 && l % LB == 0) DD_TRYP(DD_PROF_MISC, launch_graph(u.graph_at(xcur), st));   // block boundary (every launch is on this stream)
    // ---- projections of the old h / h_bond
    DD_TRYP(DD_PROF_GEMM, launch_gemm128(u.n1(l, w.h), st));
    DD_TRYP(DD_PROF_GEMM, launch_gemm128(u.l1(l, w.h), st));
    DD_TRYP(DD_PROF_GEMM, launch_gemm128(u.b1(l), st));
    DD_TRYP(DD_PROF_ASSEMBLE, launch_bl_assemble(u.assemble(l, xcur, w.q1bl), st));
    // ---- queries: second Linear of the q MLPs (LayerNorm+ReLU prologue)
    DD_TRYP(DD_PROF_GEMM, launch_gemm128(u.q_ne(l), st));
    DD_TRYP(DD_PROF_GEMM, launch_gemm128(u.q_nb(l), st));
    DD_TRYP(DD_PROF_GEMM, launch_gemm128(u.q_bl(l, false), st));
    // ---- node_layer_with_edge (no persistent workgroups)
    AttnArgs a = u.attn_ne(l, xcur, false);
    a.work_counter = nullptr;
    DD_TRYP(DD_PROF_ATTN_NE, attn_dispatch(M_NE, a, st));
    // ---- node_layer_with_bond (adds into the ligand rows of A)
    a = u.attn_nb(l, xcur);
    a.out = w.A; a.out_assign = 0;
    DD_TRYP(DD_PROF_ATTN_NB, attn_dispatch(M_NB, a, st));
    // ---- bond_layer (residual add into h_bond; small ligands: the fused launch's persistent cooperative workgroups)
    DD_TRYP(DD_PROF_ATTN_BL, attn_dispatch(M_BL, u.attn_bl(l, xcur), st));
    // ---- h += lin_node(A)
    DD_TRYP(DD_PROF_GEMM, launch_gemm128(u.lin(l, w.h, nullptr), st));
    // ---- projections of the new h / h_bond
    DD_TRYP(DD_PROF_GEMM, launch_gemm128(u.n2(l, w.h), st));
    DD_TRYP(DD_PROF_GEMM, launch_gemm128(u.l2(l, w.h), st));
    DD_TRYP(DD_PROF_GEMM, launch_gemm128(u.b2(l), st));
    // ---- pos_layer_with_edge
    DD_TRYP(DD_PROF_GEMM, launch_gemm128(u.q_pe(l), st));
    DD_TRYP(DD_PROF_ATTN_PE, attn_dispatch(M_PE, u.attn_pe(l, xcur), st));
    // ---- pos_layer_with_bond + coordinate update (ligand rows only: mask_ligand_atom)
    DD_TRYP(DD_PROF_GEMM, launch_gemm128(u.q_pb(l), st));
    a = u.attn_pb(l, xcur);
    a.out = nullptr; a.dxe = w.dxe; a.x_next = xnext;
    DD_TRYP(DD_PROF_ATTN_PB, attn_dispatch(M_PB, a, st));
    float* t = xcur; xcur = xnext; xnext = t;
  }
  if (head_join) {                                     // (no layer consumed the graph)
    if (hipStreamWaitEvent(st, dc.ev_join[8], 0) != hipSuccess) return DD_ERR_HIP;
    head_join = false;
  }
  // heads, first Linear, where the last layer's projection launch did not carry them
  if (!heads_done) {
    const float* const anb_last = lin_in_node ? f.anb_buf(L - 1) : nullptr;   // (lin_in_node: the last layer's W_lin . A_nb is pending)
    GemmList j;
    j.add(pre_att ? f.add_anb(f.pre_att_p(bh, hcur), anb_last, false) : f.bond_head1());
    j.add(f.add_anb(f.v_head1(hcur), anb_last, false));
    DD_TRYP(DD_PROF_GEMM, j.launch(st));
  }
  {
    if (hcur != w.h && hipMemcpyAsync(w.h, hcur, sizeof(float) * (size_t)B * N * 128, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return DD_ERR_HIP;                                   // (odd number of ping-pong moves: the final h where dd_workspace_view reports it)
  }
  DD_TRY(flush_pos());                                   // last layer's coordinate launch (recorded after the head GEMMs)
  if (pending_join >= 0) {
    if (hipStreamWaitEvent(st, dc.ev_join[pending_join], 0) != hipSuccess) return DD_ERR_HIP;
    pending_join = -1;
  }
  // x0-hat = ligand rows of the final x
  if (!s->pred_pos) return DD_ERR_BAD_ARG;
  // pre_att: the bond head's hidden rows need the final coordinates -- the last launch of the forward, right in front of the
  // step kernel (or dd_forward's logits) that reads them; P was formed with the heads' first Linear above
  if (xup_prev != nullptr) {                             // folded tail: the step kernel applies the update and extracts
    if (pre_att) DD_TRYP(DD_PROF_GEMM, launch_bond_head_pre_att(s, w, bh, xup_prev, w.dxe, w.dxb, NP, st));
    fold->xprev = xup_prev;
    return DD_OK;
  }
  DD_TRYP(DD_PROF_MISC, launch_extract_ligand(xcur, B, NP, NL, s->pred_pos, st));
  if (pre_att) DD_TRYP(DD_PROF_GEMM, launch_bond_head_pre_att(s, w, bh, s->pred_pos, nullptr, nullptr, 0, st));
  return DD_OK;
}

// Drift gradients of the enabled guidance terms into w.ga / w.gc / w.gr / w.gq, evaluated at x_t BEFORE the position update
// (decompdiff.py:638-677); NULL where a term is off.  profiled: the launches count towards dd_profile_step's step category.
// restraints: the chain's distance restraints or NULL; their kernel reads the run state (counter_bias as the step kernels').
struct DriftGrads { const float *ga = nullptr, *gc = nullptr, *gr = nullptr, *gq = nullptr; int scale_q = 0; };
static int launch_drifts(const dd_sampler* s, const Workspace& w, bool profiled, hipStream_t st, DriftGrads* d,
                         const RestraintArgs* restraints = nullptr, int counter_bias = 0) {
  const int B = s->B, NL = s->NL;
  auto run = [&](auto&& launch) -> int {
    ProfScope prof_scope(DD_PROF_STEP, st, profiled);
    return launch();
  };
  if (s->drift_armsca) {
    if (!s->decomp_index) return DD_ERR_BAD_ARG;
    DD_TRY(run([&] { return launch_drift_armsca(s->lig_pos, s->decomp_index, B, NL, s->armsca_min_d, s->armsca_max_d, w.ga, 0,
                                                s->drift_norm_batch, st); }));
    d->ga = w.ga;
  }
  if (s->drift_clash) {
    if (!s->full_protein_pos || s->NF <= 0) return DD_ERR_BAD_ARG;
    DD_TRY(run([&] { return launch_drift_clash(s->lig_pos, s->offset, s->full_protein_pos, B, NL, s->NF, s->clash_sigma, s->clash_gamma,
                                               w.gc, 0, s->nl_real, st); }));
    d->gc = w.gc;
  }
  if (s->drift_repul) {
    if (!s->decomp_index || (s->drift_repul != 1 && s->drift_repul != 2)) return DD_ERR_BAD_ARG;
    DD_TRY(run([&] { return launch_drift_arms_repul(s->lig_pos, s->decomp_index, B, NL, s->repul_max_d, s->drift_repul, w.gr, 0,
                                                    s->drift_norm_batch, st); }));
    d->gr = w.gr;
  }
  if (restraints) {
    RestraintArgs q = *restraints;
    q.pos = s->lig_pos; q.decomp = s->decomp_index; q.nl_real = s->nl_real; q.step_counter = s->step_counter;
    q.counter_bias = counter_bias; q.grad = w.gq; q.accumulate = 0; q.dist = nullptr; q.winner = nullptr;
    q.lig_v = s->lig_v; q.winner2 = nullptr;               // (typed restraints: the sampler's own atom classes)
    DD_TRY(run([&] { return launch_drift_restraint(q, st); }));
    d->gq = w.gq; d->scale_q = q.scale;
  }
  return DD_OK;
}

// The sampler's part of the step kernels' arguments: atom rows `r`, bond rows `rb`, positions `p`.  The callers add where the
// head outputs come from (hid / W2 / b2 or logits_in), logits_out, x0 and, with a folded step boundary, counter_bias and x0_*.
// sample_keys: the per-sample noise keys of a keyed chain (the kernels read them at every launch), NULL otherwise.
// fixed: the fixed atoms of the chain (device pointers, read at every launch), NULL otherwise.
// epoch: the resampling epoch of a chain with fixed atoms (a device int, read at every launch), NULL otherwise.
static void fill_step_args(const dd_sampler* s, const DriftGrads& d, const uint64_t* sample_keys, const dd_fixed* fixed, StepRowsArgs* r,
                           StepRowsArgs* rb, StepPosArgs* p, const int32_t* epoch = nullptr) {
  const int B = s->B, NL = s->NL;
  const long Eb = (long)NL * (NL - 1);
  memset(r, 0, sizeof(*r));
  r->rows = B * NL; r->NC = num_v(s); r->rows_per_sample = NL;
  r->tab = s->tab_v; r->T = s->T; r->step_counter = s->step_counter;
  r->state = s->lig_v; r->uniforms = s->u_v; r->stream_id = 1;
  r->traj_recon = s->traj_v0; r->traj_prob = s->traj_vt; r->traj_state = s->traj_v;
  r->sample_keys = sample_keys; r->NL = NL;
  if (fixed) { r->fx_mask = fixed->mask; r->fx_mode = fixed->mode; r->epoch = epoch; }
  *rb = *r;
  if (fixed) { r->fx_val = fixed->v0; rb->fx_val = fixed->b0; rb->fx_bond = 1; }
  rb->rows = (int)(B * Eb); rb->NC = DD_NUM_B; rb->rows_per_sample = (int)Eb; rb->tab = s->tab_b;
  rb->state = s->lig_bond; rb->uniforms = s->u_b; rb->stream_id = 2;
  rb->traj_recon = nullptr; rb->traj_prob = s->traj_bt; rb->traj_state = s->traj_bond;
  rb->nl_real = s->nl_real;                              // (keyed bond rows of a padded batch: the sample's own enumeration)
  memset(p, 0, sizeof(*p));
  p->B = B; p->NL = NL; p->T = s->T; p->step_counter = s->step_counter; p->NP = s->NP;
  p->xt = s->lig_pos; p->tab_pos = s->tab_pos; p->tab_score = s->tab_score;
  p->atom_std = s->atom_std; p->offset = s->offset; p->grad_a = d.ga; p->scale_a = s->armsca_scale; p->grad_c = d.gc;
  p->scale_c = s->clash_scale; p->grad_r = d.gr; p->scale_r = s->repul_scale; p->grad_q = d.gq; p->scale_q = d.scale_q; p->eps = s->eps; p->traj_pos = s->traj_pos;
  p->sample_keys = sample_keys;
  if (fixed) { p->fx_mask = fixed->mask; p->fx_x0c = fixed->x0c; p->fx_cc = fixed->cc; p->fx_tab = fixed->tab; p->fx_mode = fixed->mode; p->epoch = epoch; }
}

static int heads_and_step(const dd_sampler* s, hipStream_t st, const StepFold* fold, const StepExtras& x) {
  const Fwd f(s);
  const Workspace& w = f.w;
  const bool advanced = fold && fold->advance;
  DriftGrads d;
  DD_TRY(launch_drifts(s, w, true, st, &d, x.has_restraints ? &x.restraints : nullptr, advanced ? 1 : 0));
  StepRowsArgs r, rb;
  StepPosArgs p;
  fill_step_args(s, d, x.sample_keys, x.has_fixed ? &x.fixed : nullptr, &r, &rb, &p, x.epoch);
  r.counter_bias = rb.counter_bias = p.counter_bias = advanced ? 1 : 0;
  r.hid = w.qn; r.W2 = f.GW(DD_G_VH_W2); r.b2 = f.GW(DD_G_VH_b2); r.logits_out = s->pred_v;
  rb.hid = w.qb; rb.W2 = f.GW(DD_G_BH_W2); rb.b2 = f.GW(DD_G_BH_b2); rb.logits_out = s->pred_bond;
  p.x0 = s->pred_pos;
  if (fold && fold->xprev) { p.x0_prev = fold->xprev; p.x0_dxe = w.dxe; p.x0_dxb = w.dxb; p.x0_out = s->pred_pos; }
  if (g_step_fused) {
    DD_TRYP(DD_PROF_STEP, launch_step_all(rb, r, p, st));
    if (!advanced) DD_TRYP(DD_PROF_STEP, launch_advance(s->step_counter, st));
  } else {
    DD_TRYP(DD_PROF_STEP, launch_step_rows(r, st));
    DD_TRYP(DD_PROF_STEP, launch_step_rows(rb, st));
    DD_TRYP(DD_PROF_STEP, launch_step_pos(p, st));
    if (!advanced) DD_TRYP(DD_PROF_STEP, launch_advance(s->step_counter, st));
  }
  return DD_OK;
}

// One reverse step from head outputs the host computed itself (dd_reverse_step): the transitions of heads_and_step
// without the network -- unfused launches, the step counter advanced behind them.
static int reverse_step_from_logits(const dd_sampler* s, const float* logits_v, const float* logits_b, const float* x0, hipStream_t st) {
  const Workspace w = carve(s->workspace, s->B, s->NP, s->NL, s->K);
  DriftGrads d;
  DD_TRY(launch_drifts(s, w, false, st, &d));
  StepRowsArgs r, rb;
  StepPosArgs p;
  fill_step_args(s, d, nullptr, nullptr, &r, &rb, &p);
  r.logits_in = logits_v;
  rb.logits_in = logits_b;
  p.x0 = x0;
  DD_TRY(launch_step_rows(r, st));
  DD_TRY(launch_step_rows(rb, st));
  DD_TRY(launch_step_pos(p, st));
  DD_TRY(launch_advance(s->step_counter, st));
  return DD_OK;
}

// dd_fixed_init: the held rows' state in front of the first step (dd_step.hip::k_fixed_init)
static int fixed_init(const dd_sampler* s, const uint64_t* sample_keys, const dd_fixed* fixed, hipStream_t st) {
  DriftGrads d;
  StepRowsArgs r, rb;
  StepPosArgs p;
  fill_step_args(s, d, sample_keys, fixed, &r, &rb, &p);
  return launch_fixed_init(rb, r, p, st);
}

// dd_chain_init: the chain's level in front of its first step, every real row (dd_step.hip::k_chain_init)
static int chain_init(const dd_sampler* s, const uint64_t* sample_keys, const dd_init* in, hipStream_t st) {
  DriftGrads d;
  StepRowsArgs r, rb;
  StepPosArgs p;
  fill_step_args(s, d, sample_keys, nullptr, &r, &rb, &p);
  ChainInitArgs ci;
  ci.mode = in->mode; ci.cc = in->cc; ci.std = in->std; ci.lp_v = in->atom_log_prior; ci.lp_b = in->bond_log_prior;
  ci.x0c = in->x0c; ci.v0 = in->v0; ci.b0 = in->b0; ci.tab = in->tab; ci.nl_real = s->nl_real;
  return launch_chain_init(rb, r, p, ci, st);
}

// dd_resample_jump: the forward jump of the chain's state and the rebase of its run state (dd_step.hip::k_jump)
static int resample_jump(const dd_sampler* s, const uint64_t* sample_keys, const dd_fixed* fixed, const dd_resample* rsm, hipStream_t st) {
  DriftGrads d;
  StepRowsArgs r, rb;
  StepPosArgs p;
  fill_step_args(s, d, sample_keys, fixed, &r, &rb, &p, rsm->epoch);
  return launch_jump(rb, r, p, rsm->tab, rsm->jump_length, rsm->epoch, st);
}

// forward-only head evaluation: logits without sampling (state untouched)
__global__ __launch_bounds__(256) void k_head_logits(const float* __restrict__ hid, const float* __restrict__ W2,
                                                     const float* __restrict__ b2, int rows, int NC,
                                                     float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float2 hv = *reinterpret_cast<const float2*>(hid + row * 128 + 2 * lane);
  hv.x = (hv.x > 20.f ? hv.x : log1pf(expf(hv.x))) - 0.6931471805599453f;
  hv.y = (hv.y > 20.f ? hv.y : log1pf(expf(hv.y))) - 0.6931471805599453f;
  for (int c = 0; c < NC; ++c) {
    const float2 w = *reinterpret_cast<const float2*>(W2 + c * 128 + 2 * lane);
    float v = wave_sum(fmaf(hv.y, w.y, hv.x * w.x)) + b2[c];
    if (lane == 0) out[row * NC + c] = v;
  }
}

}  // namespace dd

extern "C" const char* dd_status_string(int status) {
  switch (status) {
    case DD_OK: return "ok";
    case DD_ERR_BAD_ARG: return "bad argument (null pointer or non-positive size)";
    case DD_ERR_UNSUPPORTED_SHAPE: return "unsupported shape (NL > 128, N > 2048, K > 64 or K > N-1)";
    case DD_ERR_WORKSPACE_TOO_SMALL: return "workspace too small (see dd_workspace_floats)";
    case DD_ERR_HIP: return "HIP launch/runtime error";
  }
  return "unknown status";
}

// 3: tab_v / tab_b carry the class log-prior after the four schedule rows
// 4: step_counter is the [4] int32 run state (steps done, t_start, seed lo, seed hi) written by dd_sampler_reset
// 5: np_real / nl_real / bl_prefix (padded heterogeneous batches) appended to dd_sampler
// 7: dd_queue_error; the workspace carries the layer-tail queue's flag words (dd_workspace_floats grew)
// 8: arms_repul drift (dd_sampler.drift_repul / repul_max_d / repul_scale, dd_drift_arms_repul; the workspace grew by one
//    gradient buffer); dd_build_flags
extern "C" int dd_abi_version(void) { return 9; }
extern "C" int dd_build_flags(void) {
  int f = 0;
#if defined(DD_DEBUG_OPTIONS) && DD_DEBUG_OPTIONS
  f |= 1;
#endif
#if defined(DD_EXACT_MATH) && DD_EXACT_MATH
  f |= 2;
#endif
  return f;
}

// 6: l0_tables / l0_P / l0_qn (layer-0 tables) appended to dd_sampler
extern "C" int dd_layer0_tables(const dd_sampler* m, float* tables, void* stream) {
  if (!m || !tables || !m->weights || !m->slot_off || !m->workspace || !m->lig_v || !m->lig_aux || !m->lig_bond || !m->lig_pos)
    return DD_ERR_BAD_ARG;
  if (m->B != 1 || m->NP != 0 || m->NL != 16 || dd::num_v(m) != DD_NUM_V) return DD_ERR_BAD_ARG;   // (16 = DD_NUM_V classes x arm flag)
  int rc = dd::check_shapes(m);
  if (rc != DD_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const dd::Fwd f(m);
  const dd::Workspace& w = f.w;
  if ((rc = dd::launch_embed(f.embed(nullptr), st)) != DD_OK) return rc;
  if ((rc = f.launch_projections1(0, w.h, st)) != DD_OK) return rc;
  if ((rc = f.launch_queries(0, true, st)) != DD_OK) return rc;
  // atom i has combination i; bonds dst*15 + s have type s % 5 (s < 5: type s)
  auto cp = [&](float* dst, const float* src, size_t n) {
    return hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess;
  };
  bool ok = cp(tables, w.P, 16 * 640) && cp(tables + 16 * 640, w.PL, 16 * 1280) && cp(tables + 16 * 640 + 16 * 1280, w.PB, 5 * 640);
  float* tq = tables + 16 * 640 + 16 * 1280 + 5 * 640;
  ok = ok && cp(tq, w.qn, 16 * 128) && cp(tq + 16 * 128, w.qlnb, 16 * 128);
  for (int c = 0; c < 16 && ok; ++c) ok = cp(tq + 32 * 128 + (size_t)c * 5 * 128, w.qb + (size_t)c * 15 * 128, 5 * 128);
  return ok ? DD_OK : DD_ERR_HIP;
}

extern "C" int dd_layer0_prepare(const dd_sampler* s, void* stream) {
  if (!s || !s->weights || !s->slot_off || !s->l0_P || !s->l0_qn) return DD_ERR_BAD_ARG;
  if (s->NP <= 0) return DD_OK;
  if (!s->protein_h) return DD_ERR_BAD_ARG;
  // the protein rows of the layer-0 node projections and node queries: same GEMM tile code, rows mapped into the [B, N] tables
  const dd::Fwd f(s);
  const dd::GemmArgs g1 = f.n1_l0_protein(), g2 = f.q_ne_l0_protein();
  int rc = dd::launch_gemm128_batch(&g1, 1, (hipStream_t)stream);
  if (rc != DD_OK) return rc;
  return dd::launch_gemm128_batch(&g2, 1, (hipStream_t)stream);
}

extern "C" int dd_sampler_reset(const dd_sampler* s, void* stream) {
  if (!s || !s->step_counter) return DD_ERR_BAD_ARG;
  if (s->t_start < 0 || s->t_start >= s->T) return DD_ERR_BAD_ARG;
  return dd::launch_reset_run_state(s->step_counter, s->t_start, s->seed, (hipStream_t)stream);
}

extern "C" size_t dd_workspace_floats(int B, int NP, int NL, int K) {
  if (B <= 0 || NP < 0 || NL <= 0 || K <= 0) return 0;
  return dd::carve(nullptr, B, NP, NL, K).total;
}

// The descriptors and the block count of a dd_model_opts (NULL: one block, no descriptors).  `size` is the caller's
// sizeof(dd_model_opts): fields beyond it are not read, so a caller built against a shorter struct keeps working.
static int read_model_opts(const dd_model_opts* o, dd::ModelOpts* mo) {
  *mo = dd::ModelOpts();
  if (o == nullptr) return DD_OK;
  const size_t size = o->size > 0 ? (size_t)o->size : 0;
  auto has = [&](size_t off, size_t n) { return size >= off + n; };
  if (!has(0, sizeof(int32_t))) return DD_ERR_BAD_ARG;
  if (has(offsetof(dd_model_opts, bond_head), sizeof(o->bond_head))) mo->bh = o->bond_head;
  if (has(offsetof(dd_model_opts, node_out), sizeof(o->node_out))) mo->no = o->node_out;
  if (has(offsetof(dd_model_opts, num_blocks), sizeof(o->num_blocks))) mo->num_blocks = o->num_blocks;
  return mo->num_blocks >= 1 ? DD_OK : DD_ERR_BAD_ARG;
}
// ... checked against the sampler (what every entry point that runs the network asks first)
static int check_model(const dd_sampler* s, const dd::ModelOpts& mo) {
  if (dd::check_bond_head(mo.bh) != DD_OK || dd::check_node_out(mo.no, s) != DD_OK) return DD_ERR_BAD_ARG;
  return dd::check_blocks(s, mo.num_blocks);
}
static dd_model_opts opts_of(const dd_bond_head* bh, const dd_node_out* no) {
  dd_model_opts o;
  o.size = (int32_t)sizeof(dd_model_opts); o.bond_head = bh; o.node_out = no; o.num_blocks = 1;
  return o;
}

extern "C" int dd_workspace_view(const dd_sampler* s, dd_ws_view* out) { return dd_workspace_view_opts(s, nullptr, out); }

extern "C" int dd_workspace_view_opts(const dd_sampler* s, const dd_model_opts* opts, dd_ws_view* out) {
  if (!s || !out || !s->workspace) return DD_ERR_BAD_ARG;
  dd::ModelOpts mo;
  if (read_model_opts(opts, &mo) != DD_OK) return DD_ERR_BAD_ARG;
  const int steps = mo.num_blocks * s->num_layers;       // x and Anb ping-pong by the step
  dd::Workspace w = dd::carve(s->workspace, s->B, s->NP, s->NL, s->K);
  out->x = (steps & 1) ? w.xb : w.xa;
  out->h = w.h; out->hb = w.hb; out->ew = w.ew; out->A = w.A; out->nbr = w.nbr;
  out->Anb = (dd::g_fuse && s->NL <= dd::g_fused_max_nl) ? w.Anb : nullptr;
  out->lin_in_node = 0;
  if (dd::uses_lin_in_node(s->B, s->NL, mo.no != nullptr, out->Anb != nullptr)) {
    // lin_node inside the node launch: `h` lacks the last layer's W_lin . A_nb on the ligand rows -- it is in `Anb`; `A` is not formed
    out->lin_in_node = 1;
    out->Anb = ((steps - 1) & 1) ? w.A : w.Anb;
    out->A = nullptr;
  }
  return DD_OK;
}

extern "C" int dd_forward(const dd_sampler* s, void* stream) { return dd_forward_ex(s, nullptr, stream); }

extern "C" int dd_forward_ex(const dd_sampler* s, const dd_bond_head* bh, void* stream) { return dd_forward_ex2(s, bh, nullptr, stream); }

extern "C" int dd_forward_ex2(const dd_sampler* s, const dd_bond_head* bh, const dd_node_out* no, void* stream) {
  const dd_model_opts o = opts_of(bh, no);
  return dd_forward_opts(s, &o, stream);
}

extern "C" int dd_forward_opts(const dd_sampler* s, const dd_model_opts* opts, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  dd::ModelOpts mo;
  int rc = read_model_opts(opts, &mo);
  if (rc != DD_OK) return rc;
  rc = dd::check_bond_head(mo.bh);
  if (rc != DD_OK) return rc;
  rc = dd::forward_impl(s, st, nullptr, mo);
  if (rc != DD_OK) return rc;
  if (!s->pred_pos || !s->pred_v || !s->pred_bond) return DD_ERR_BAD_ARG;
  const dd::Fwd f(s);
  const dd::Workspace& w = f.w;
  const int rows_v = s->B * s->NL;
  const long rows_b = (long)s->B * s->NL * (s->NL - 1);
  hipLaunchKernelGGL(dd::k_head_logits, dim3((rows_v + 3) / 4), dim3(256), 0, st, w.qn, f.GW(DD_G_VH_W2), f.GW(DD_G_VH_b2),
                     rows_v, dd::num_v(s), s->pred_v);
  hipLaunchKernelGGL(dd::k_head_logits, dim3((unsigned)((rows_b + 3) / 4)), dim3(256), 0, st, w.qb, f.GW(DD_G_BH_W2),
                     f.GW(DD_G_BH_b2), (int)rows_b, DD_NUM_B, s->pred_bond);
  DD_CHECK_LAUNCH();
  return DD_OK;
}

namespace dd {
extern int g_node_split_trial;
int node_split_lookup(int B, int NP, int NL, int K);
void node_split_store(int B, int NP, int NL, int K, int n_bl);
bool node_split_applies(int B, int NL, int n_cu);
}

// One-off measurement per (B, NP, NL, K): how many CUs the persistent bond-layer workgroups of the fused node launch
// keep (see launch_node_nw).  Times whole forward passes on `st` (eager, min of 2 after a warm-up pass) for a coarse and
// then a fine set of splits around the work-proportional share; ~21 forward passes, before the first graph of a shape
// is captured.  The passes only write the workspace and pred_*.
// ---- measured splits kept ACROSS processes (per device model and build of this library): eight ranks of a node, or the next
// run of the sampling script, read the file instead of each timing ~30 forward passes per shape while their neighbours do the same
// on a shared host.  One text line per shape, "B NP NL K n_bl"; the file is replaced atomically (temp + rename), a lost update only
// means that shape is measured again.  DD_NODE_SPLIT_CACHE=0 turns it off, DD_NODE_SPLIT_CACHE_DIR moves it (default
// $XDG_CACHE_HOME or ~/.cache, /decompdiff_amd).  The split never changes results (it only decides WHICH CU computes a segment).
static std::string node_split_cache_path(int n_cu) {
  const char* off = getenv("DD_NODE_SPLIT_CACHE");
  if (off && off[0] == '0') return std::string();
  std::string dir;
  if (const char* d = getenv("DD_NODE_SPLIT_CACHE_DIR")) dir = d;
  else if (const char* x = getenv("XDG_CACHE_HOME")) dir = std::string(x) + "/decompdiff_amd";
  else if (const char* h = getenv("HOME")) dir = std::string(h) + "/.cache/decompdiff_amd";
  else return std::string();
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) { (void)hipGetLastError(); return std::string(); }
  std::string name = std::string(prop.gcnArchName) + "_" + prop.name;
  for (char& c : name) if (!((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9'))) c = '_';
  unsigned h = 2166136261u;                              // the build: a rebuilt kernel is measured again
  for (const char* p = __DATE__ " " __TIME__; *p; ++p) h = (h ^ (unsigned char)*p) * 16777619u;
  char tag[64];
  snprintf(tag, sizeof(tag), "_cu%d_abi%d_%08x", n_cu, dd_abi_version(), h);
  return dir + "/node_split_" + name + tag + ".txt";
}
static int node_split_cache_read(const std::string& path, int B, int NP, int NL, int K) {
  if (path.empty()) return -1;
  FILE* f = fopen(path.c_str(), "r");
  if (!f) return -1;
  int b, np, nl, k, n, found = -1;
  while (fscanf(f, "%d %d %d %d %d", &b, &np, &nl, &k, &n) == 5)
    if (b == B && np == NP && nl == NL && k == K) found = n;         // (the last line of a shape wins)
  fclose(f);
  return found;
}
static void node_split_cache_append(const std::string& path, int B, int NP, int NL, int K, int n_bl) {
  if (path.empty()) return;
  const size_t slash = path.rfind('/');
  if (slash != std::string::npos) {
    std::string dir = path.substr(0, slash);
    for (size_t i = 1; i <= dir.size(); ++i)
      if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0755);
  }
  std::string all;
  if (FILE* f = fopen(path.c_str(), "r")) {
    char buf[256];
    while (fgets(buf, sizeof(buf), f)) all += buf;
    fclose(f);
  }
  char line[96];
  snprintf(line, sizeof(line), "%d %d %d %d %d\n", B, NP, NL, K, n_bl);
  all += line;
  char tmp[32];
  snprintf(tmp, sizeof(tmp), ".tmp%d", (int)getpid());
  const std::string t = path + tmp;
  FILE* f = fopen(t.c_str(), "w");
  if (!f) return;
  const bool ok = fwrite(all.data(), 1, all.size(), f) == all.size();
  fclose(f);
  if (!ok || rename(t.c_str(), path.c_str()) != 0) (void)unlink(t.c_str());
}

static int autotune_node_split(const dd_sampler* s, int num_blocks, hipStream_t st) {
  dd::ModelOpts mo;                                      // (the timed passes run the caller's block count, without descriptors as before)
  mo.num_blocks = num_blocks;
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return DD_ERR_HIP;
    n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  const bool fused = dd::g_fuse && s->NL <= dd::g_fused_max_nl && dd::g_dbg_clock == nullptr;
  // DD_NODE_SPLIT_AUTOTUNE=0: no measurement passes (the node blocks then simply come first in the launch)
  static const bool enabled = [] { const char* e = getenv("DD_NODE_SPLIT_AUTOTUNE"); return !(e && e[0] == '0'); }();
  if (!enabled) return DD_OK;
  if (!fused || !dd::node_split_applies(s->B, s->NL, n_cu) || dd::node_split_lookup(s->B, s->NP, s->NL, s->K) >= 0) return DD_OK;
  const std::string cache_path = node_split_cache_path(n_cu);
  {
    const int cached = node_split_cache_read(cache_path, s->B, s->NP, s->NL, s->K);
    if (cached == 0 || (cached >= 16 && cached <= n_cu - 16 && cached % 8 == 0)) {       // (anything else: measure again)
      dd::node_split_store(s->B, s->NP, s->NL, s->K, cached);
      return DD_OK;
    }
  }
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return DD_ERR_HIP;
  int rc = DD_OK;
  auto time_split = [&](int n_bl, float& best) {
    dd::g_node_split_trial = n_bl;
    best = 1e30f;
    for (int rep = 0; rep < 3 && rc == DD_OK; ++rep) {
      if (hipEventRecord(e0, st) != hipSuccess) { rc = DD_ERR_HIP; break; }
      rc = dd::forward_impl(s, st, nullptr, mo);
      if (rc != DD_OK) break;
      float ms = 0.f;
      if (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
          hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { rc = DD_ERR_HIP; break; }
      if (rep > 0 && ms < best) best = ms;                 // (the first pass of a setting warms caches)
    }
  };
  int best_n = 0;
  float best_t = 0.f, t = 0.f;
  // scan around the work-proportional share (rough unit costs: a node block of 8 centres 1.0, a bond-layer batch of 8
  // segments 0.1 + 0.35 per 16-member tile) -- far from it a candidate only costs time (a starved part runs for ms)
  const int tiles = (s->NL - 2 + 15) / 16;
  const double w_bl = ((double)s->B * s->NL * (s->NL - 1) / 8.0) * (0.1 + 0.35 * tiles);
  const double w_node = (double)s->B * ((s->NP + 7) / 8 + (s->NL + 7) / 8) + (double)s->B * s->NL / 8.0;
  const int centre = (int)(n_cu * w_bl / (w_bl + w_node)) / 8 * 8;
  // A job of many pockets (configs[3]: 100 shapes) does not scan for every shape: the measured optimum sits at a stable
  // offset from the work-proportional share within one kernel variant (tile class) and batch size, so a shape whose class
  // has been scanned before only times that prediction and its two neighbours (9 forward passes instead of ~33).
  struct Seen { int B, K, tiles, offset; };
  static std::vector<Seen> seen;
  static std::mutex seen_mutex;
  int predicted = -1;
  {
    std::lock_guard<std::mutex> lock(seen_mutex);
    for (const Seen& e : seen)
      if (e.B == s->B && e.K == s->K && e.tiles == tiles) predicted = centre + e.offset;
  }
  if (predicted >= 0) {
    predicted = predicted < 16 ? 16 : (predicted > n_cu - 16 ? n_cu - 16 : predicted);
    best_t = 1e30f;
    for (int n : {predicted, predicted - 8, predicted + 8}) {
      if (rc != DD_OK || n < 16 || n > n_cu - 16) continue;
      time_split(n, t);
      if (t < best_t) { best_t = t; best_n = n; }
    }
  } else {
    time_split(0, best_t);
    const int lo = centre - 32 < n_cu / 4 ? n_cu / 4 : centre - 32, hi = centre + 16 > n_cu - 16 ? n_cu - 16 : centre + 16;
    for (int n = lo; n <= hi && rc == DD_OK; n += 16) {
      time_split(n, t);
      if (t < best_t) { best_t = t; best_n = n; }
    }
    if (best_n > 0)
      for (int n : {best_n - 8, best_n + 8}) {
        if (rc != DD_OK || n < 16 || n > n_cu - 16) continue;
        time_split(n, t);
        if (t < best_t) { best_t = t; best_n = n; }
      }
    if (rc == DD_OK && best_n > 0) {
      std::lock_guard<std::mutex> lock(seen_mutex);
      seen.push_back(Seen{s->B, s->K, tiles, best_n - centre});
    }
  }
  dd::g_node_split_trial = -1;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc == DD_OK) {
    dd::node_split_store(s->B, s->NP, s->NL, s->K, best_n);
    node_split_cache_append(cache_path, s->B, s->NP, s->NL, s->K, best_n);
  }
  return rc;
}

extern "C" int dd_debug_node_split_cache_path(char* out, int cap) {
  if (!out || cap <= 0) return DD_ERR_BAD_ARG;
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) { (void)hipGetLastError(); return DD_ERR_HIP; }
  const std::string p = node_split_cache_path(prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256);
  if ((int)p.size() + 1 > cap) return DD_ERR_BAD_ARG;
  memcpy(out, p.c_str(), p.size() + 1);                  // (empty string: the cache is turned off)
  return DD_OK;
}

// What every entry point that takes reverse steps needs of the sampler (beside check_shapes)
static bool check_step_sampler(const dd_sampler* s) {
  return s && s->step_counter && s->tab_pos && s->tab_v && s->tab_b && s->atom_std && s->offset && s->pred_pos;
}

static int one_step(const dd_sampler* s, hipStream_t st, const dd::ModelOpts& mo = dd::ModelOpts(),
                    const dd::StepExtras& x = dd::StepExtras()) {
  dd::StepFold fold;
  fold.advance = fold.fold_tail = dd::g_step_fold != 0;
  int rc = dd::forward_impl(s, st, &fold, mo);
  if (rc != DD_OK) return rc;
  return dd::heads_and_step(s, st, &fold, x);
}

extern "C" int dd_reverse_step(const dd_sampler* s, const float* logits_v, const float* logits_b, const float* x0, void* stream) {
  if (!s || !logits_v || !logits_b || !x0 || !s->step_counter || !s->tab_pos || !s->tab_v || !s->tab_b || !s->atom_std ||
      !s->offset || !s->workspace)
    return DD_ERR_BAD_ARG;
  int rc = dd::check_shapes(s);
  if (rc != DD_OK) return rc;
  return dd::reverse_step_from_logits(s, logits_v, logits_b, x0, (hipStream_t)stream);
}

extern "C" int dd_sample_steps(const dd_sampler* s, int n_steps, void* stream) { return dd_sample_steps_ex(s, nullptr, n_steps, stream); }

extern "C" int dd_sample_steps_ex(const dd_sampler* s, const dd_bond_head* bh, int n_steps, void* stream) {
  return dd_sample_steps_ex2(s, bh, nullptr, n_steps, stream);
}

extern "C" int dd_sample_steps_ex2(const dd_sampler* s, const dd_bond_head* bh, const dd_node_out* no, int n_steps, void* stream) {
  const dd_model_opts o = opts_of(bh, no);
  return dd_sample_steps_opts(s, &o, n_steps, stream);
}

extern "C" int dd_sample_steps_opts(const dd_sampler* s, const dd_model_opts* opts, int n_steps, void* stream) {
  return dd_sample_steps_keyed(s, opts, nullptr, n_steps, stream);
}

// Per-sample noise keys exclude injected noise: a chain draws from one or the other.
static bool keys_with_injected_noise(const dd_sampler* s, const uint64_t* sample_keys) {
  return sample_keys != nullptr && s != nullptr && (s->u_v != nullptr || s->u_b != nullptr || s->eps != nullptr);
}

// The caller's dd_fixed as a checked copy (fields beyond its `size` are NULL / 0); NULL stays "no fixed atoms"
static int read_fixed(const dd_fixed* fixed, dd_fixed* out) {
  if (!dd::read_sized(fixed, out)) return DD_ERR_BAD_ARG;
  if (out->mode != DD_FIXED_HOLD && out->mode != DD_FIXED_REPLACE) return DD_ERR_BAD_ARG;
  if (!out->mask || !out->v0 || !out->b0 || !out->x0c) return DD_ERR_BAD_ARG;
  if (out->mode == DD_FIXED_REPLACE && (!out->cc || !out->tab)) return DD_ERR_BAD_ARG;
  return DD_OK;
}

extern "C" int dd_sample_steps_keyed(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, int n_steps, void* stream) {
  return dd_sample_steps_fixed(s, opts, sample_keys, nullptr, n_steps, stream);
}

// The caller's dd_resample as a checked copy: every field is needed, the chain has fixed atoms with centres (a jump noises around
// them in both modes), draws on the device, and its times fit the 16 bits of the time word below the epoch
static int read_resample(const dd_resample* rsm, const dd_sampler* s, const dd_fixed* fixed, dd_resample* out) {
  if (!dd::read_sized(rsm, out) || fixed == nullptr || s == nullptr) return DD_ERR_BAD_ARG;
  if (out->jump_length < 1 || !out->tab || !out->epoch) return DD_ERR_BAD_ARG;
  if (s->T < 1 || s->T > 65535 || s->u_v || s->u_b || s->eps) return DD_ERR_BAD_ARG;
  return DD_OK;
}

static int sample_steps_impl(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, const dd_fixed* fixed,
                             const dd_resample* rsm, const dd_restraints* rst, int n_steps, void* stream);

extern "C" int dd_sample_steps_fixed(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, const dd_fixed* fixed,
                                     int n_steps, void* stream) {
  return sample_steps_impl(s, opts, sample_keys, fixed, nullptr, nullptr, n_steps, stream);
}

extern "C" int dd_sample_steps_resample(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, const dd_fixed* fixed,
                                        const dd_resample* resample, int n_steps, void* stream) {
  if (!resample) return DD_ERR_BAD_ARG;
  return dd_sample_steps_guided(s, opts, sample_keys, fixed, resample, nullptr, n_steps, stream);
}

// The last of the suffix chain: keys, fixed atoms, resampling and distance restraints, each NULL-able
extern "C" int dd_sample_steps_guided(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, const dd_fixed* fixed,
                                      const dd_resample* resample, const dd_restraints* restraints, int n_steps, void* stream) {
  return sample_steps_impl(s, opts, sample_keys, fixed, resample, restraints, n_steps, stream);
}

// What the step entry points take beside their step count, read and checked in one place, each of the last four NULL-able: the
// model against the sampler, the keys (a keyed chain draws on the device), the fixed atoms, the resampling schedule (it needs fixed
// atoms) and the restraints (checked against the sampler; their arrays are fetched on `st` and waited for).  capture: a graph is
// about to be captured from `st`, which must then be a real stream, and an unsupported shape is reported before the restraints
// are fetched -- the eager loop learns of one in its first forward.
static int read_step_extras(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, const dd_fixed* fixed,
                            const dd_resample* rsm, const dd_restraints* rst, hipStream_t st, bool capture, dd::ModelOpts* mo,
                            dd::StepExtras* x) {
  *x = dd::StepExtras();
  if (read_model_opts(opts, mo) != DD_OK || check_model(s, *mo) == DD_ERR_BAD_ARG) return DD_ERR_BAD_ARG;
  if (!check_step_sampler(s) || keys_with_injected_noise(s, sample_keys)) return DD_ERR_BAD_ARG;
  if (fixed != nullptr && read_fixed(fixed, &x->fixed) != DD_OK) return DD_ERR_BAD_ARG;
  dd_resample rs;
  if (rsm != nullptr && read_resample(rsm, s, fixed, &rs) != DD_OK) return DD_ERR_BAD_ARG;
  x->sample_keys = sample_keys;
  x->has_fixed = fixed != nullptr;
  x->epoch = rsm != nullptr ? rs.epoch : nullptr;
  if (capture) {
    if (st == nullptr) return DD_ERR_BAD_ARG;    // the legacy default stream cannot be captured
    const int rc = dd::check_shapes(s);
    if (rc != DD_OK) return rc;
  }
  if (rst == nullptr) return DD_OK;
  if (!s->workspace || !s->lig_pos) return DD_ERR_BAD_ARG;
  const int rc = dd::read_restraints(rst, s->B, s->NL, s->decomp_index != nullptr, s->lig_v != nullptr, true, st, &x->restraints);
  if (rc != DD_OK) return rc;
  x->has_restraints = true;
  return x->restraints.t_min < 0 || x->restraints.t_max >= s->T ? DD_ERR_BAD_ARG : DD_OK;
}

static int sample_steps_impl(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, const dd_fixed* fixed,
                             const dd_resample* rsm, const dd_restraints* rst, int n_steps, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  dd::ModelOpts mo;
  dd::StepExtras x;
  if (n_steps < 0) return DD_ERR_BAD_ARG;
  int rc = read_step_extras(s, opts, sample_keys, fixed, rsm, rst, st, false, &mo, &x);
  for (int i = 0; i < n_steps && rc == DD_OK; ++i) rc = one_step(s, st, mo, x);
  return rc;
}

extern "C" int dd_sample_steps_graph(const dd_sampler* s, int n_steps, void* stream) {
  return dd_sample_steps_graph_ex(s, nullptr, n_steps, stream);
}

extern "C" int dd_sample_steps_graph_ex(const dd_sampler* s, const dd_bond_head* bh, int n_steps, void* stream) {
  return dd_sample_steps_graph_ex2(s, bh, nullptr, n_steps, stream);
}

// `steps` reverse steps of `s` captured from `st` into a graph and instantiated.  Measures the node split of the shape first
// (eager passes), then holds the capture mutex while the stream captures: the side stream / events of the device are shared.
// On any failure nothing is left behind: what was made is destroyed, *graph / *exec are NULL and the sticky HIP error is cleared.
static int capture_steps(const dd_sampler* s, const dd::ModelOpts& mo, const dd::StepExtras& x, int steps, hipStream_t st,
                         hipGraph_t* graph, hipGraphExec_t* exec) {
  *graph = nullptr;
  *exec = nullptr;
  int rc = autotune_node_split(s, mo.num_blocks, st);
  if (rc != DD_OK) return rc;
  {
    std::lock_guard<std::mutex> capture_lock(dd::g_capture_mutex);
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
      (void)hipGetLastError();                     // do not leave a sticky error behind for the caller
      return DD_ERR_HIP;
    }
    for (int i = 0; i < steps && rc == DD_OK; ++i) rc = one_step(s, st, mo, x);
    if (hipStreamEndCapture(st, graph) != hipSuccess || !*graph) rc = rc != DD_OK ? rc : DD_ERR_HIP;
  }
  if (rc == DD_OK && hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0) != hipSuccess) rc = DD_ERR_HIP;
  if (rc != DD_OK) {
    if (*graph) (void)hipGraphDestroy(*graph);
    *graph = nullptr;
    *exec = nullptr;
    (void)hipGetLastError();
  }
  return rc;
}

extern "C" int dd_sample_steps_graph_ex2(const dd_sampler* s, const dd_bond_head* bh, const dd_node_out* no, int n_steps, void* stream) {
  const dd_model_opts o = opts_of(bh, no);
  return dd_sample_steps_graph_opts(s, &o, n_steps, stream);
}

extern "C" int dd_sample_steps_graph_opts(const dd_sampler* s, const dd_model_opts* opts, int n_steps, void* stream) {
  dd::ModelOpts mo;
  if (read_model_opts(opts, &mo) != DD_OK || check_model(s, mo) == DD_ERR_BAD_ARG) return DD_ERR_BAD_ARG;
  if (!check_step_sampler(s) || n_steps < 0) return DD_ERR_BAD_ARG;
  if (n_steps == 0) return DD_OK;
  hipStream_t st = (hipStream_t)stream;
  int rc = dd::check_shapes(s);
  if (rc != DD_OK) return rc;
  if (st == nullptr) return DD_ERR_BAD_ARG;      // the legacy default stream cannot be captured
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  rc = capture_steps(s, mo, dd::StepExtras(), 1, st, &graph, &exec);
  if (rc != DD_OK) return rc;
  for (int i = 0; i < n_steps; ++i) {
    if (hipGraphLaunch(exec, st) != hipSuccess) { rc = DD_ERR_HIP; break; }
  }
  // the exec object must outlive its launches: wait for this stream only, then release
  if (hipStreamSynchronize(st) != hipSuccess) rc = DD_ERR_HIP;
  (void)hipGraphExecDestroy(exec);
  (void)hipGraphDestroy(graph);
  return rc;
}

namespace { struct StepGraph { unsigned magic = 0x44444753u; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; }; }

extern "C" int dd_graph_create(const dd_sampler* s, int steps_per_graph, void* stream, void** graph_out) {
  return dd_graph_create_ex(s, nullptr, steps_per_graph, stream, graph_out);
}

extern "C" int dd_graph_create_ex(const dd_sampler* s, const dd_bond_head* bh, int steps_per_graph, void* stream, void** graph_out) {
  return dd_graph_create_ex2(s, bh, nullptr, steps_per_graph, stream, graph_out);
}

extern "C" int dd_graph_create_ex2(const dd_sampler* s, const dd_bond_head* bh, const dd_node_out* no, int steps_per_graph, void* stream,
                                   void** graph_out) {
  const dd_model_opts o = opts_of(bh, no);
  return dd_graph_create_opts(s, &o, steps_per_graph, stream, graph_out);
}

extern "C" int dd_graph_create_opts(const dd_sampler* s, const dd_model_opts* opts, int steps_per_graph, void* stream, void** graph_out) {
  return dd_graph_create_keyed(s, opts, nullptr, steps_per_graph, stream, graph_out);
}

extern "C" int dd_graph_create_keyed(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, int steps_per_graph,
                                     void* stream, void** graph_out) {
  return dd_graph_create_fixed(s, opts, sample_keys, nullptr, steps_per_graph, stream, graph_out);
}

extern "C" int dd_fixed_init(const dd_sampler* s, const uint64_t* sample_keys, const dd_fixed* fixed, void* stream) {
  if (!check_step_sampler(s) || !fixed || !s->lig_pos || !s->lig_v || !s->lig_bond) return DD_ERR_BAD_ARG;
  dd_fixed fx;
  if (read_fixed(fixed, &fx) != DD_OK || keys_with_injected_noise(s, sample_keys)) return DD_ERR_BAD_ARG;
  // replace draws level t_start itself: a chain with injected noise supplies that level, and the level must exist
  if (fx.mode == DD_FIXED_REPLACE && (s->u_v || s->u_b || s->eps || s->t_start < 0 || s->t_start >= s->T)) return DD_ERR_BAD_ARG;
  int rc = dd::check_shapes(s);
  if (rc != DD_OK) return rc;
  return dd::fixed_init(s, sample_keys, &fx, (hipStream_t)stream);
}

// The caller's dd_init as a checked copy (fields beyond its `size` are NULL / 0)
static int read_init(const dd_init* init, dd_init* out) {
  if (!dd::read_sized(init, out)) return DD_ERR_BAD_ARG;
  if (out->mode != DD_INIT_PRIOR && out->mode != DD_INIT_NOISED) return DD_ERR_BAD_ARG;
  if (!out->cc || !out->std) return DD_ERR_BAD_ARG;
  if (out->mode == DD_INIT_NOISED && (!out->x0c || !out->v0 || !out->b0 || !out->tab)) return DD_ERR_BAD_ARG;
  return DD_OK;
}

extern "C" int dd_chain_init(const dd_sampler* s, const uint64_t* sample_keys, const dd_init* init, void* stream) {
  if (!check_step_sampler(s) || !init || !s->lig_pos || !s->lig_v || !s->lig_bond) return DD_ERR_BAD_ARG;
  dd_init in;
  if (read_init(init, &in) != DD_OK) return DD_ERR_BAD_ARG;
  // the level is drawn here: a chain with injected noise supplies its own, and a noised level must exist
  if (s->u_v || s->u_b || s->eps || s->T < 1) return DD_ERR_BAD_ARG;
  if (in.mode == DD_INIT_NOISED && (s->t_start < 0 || s->t_start >= s->T)) return DD_ERR_BAD_ARG;
  int rc = dd::check_shapes(s);
  if (rc != DD_OK) return rc;
  return dd::chain_init(s, sample_keys, &in, (hipStream_t)stream);
}

static int graph_create_impl(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, const dd_fixed* fixed,
                             const dd_resample* rsm, const dd_restraints* rst, int steps_per_graph, void* stream, void** graph_out);

extern "C" int dd_graph_create_fixed(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, const dd_fixed* fixed,
                                     int steps_per_graph, void* stream, void** graph_out) {
  return graph_create_impl(s, opts, sample_keys, fixed, nullptr, nullptr, steps_per_graph, stream, graph_out);
}

extern "C" int dd_graph_create_resample(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, const dd_fixed* fixed,
                                        const dd_resample* resample, int steps_per_graph, void* stream, void** graph_out) {
  if (!resample) return DD_ERR_BAD_ARG;
  return dd_graph_create_guided(s, opts, sample_keys, fixed, resample, nullptr, steps_per_graph, stream, graph_out);
}

extern "C" int dd_graph_create_guided(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, const dd_fixed* fixed,
                                      const dd_resample* resample, const dd_restraints* restraints, int steps_per_graph, void* stream,
                                      void** graph_out) {
  return graph_create_impl(s, opts, sample_keys, fixed, resample, restraints, steps_per_graph, stream, graph_out);
}

extern "C" int dd_resample_jump(const dd_sampler* s, const uint64_t* sample_keys, const dd_fixed* fixed, const dd_resample* resample,
                                void* stream) {
  if (!check_step_sampler(s) || !fixed || !resample || !s->lig_pos || !s->lig_v || !s->lig_bond) return DD_ERR_BAD_ARG;
  dd_fixed fx;
  dd_resample rs;
  if (read_fixed(fixed, &fx) != DD_OK || !fx.cc || read_resample(resample, s, fixed, &rs) != DD_OK) return DD_ERR_BAD_ARG;
  if (keys_with_injected_noise(s, sample_keys)) return DD_ERR_BAD_ARG;
  int rc = dd::check_shapes(s);
  if (rc != DD_OK) return rc;
  return dd::resample_jump(s, sample_keys, &fx, &rs, (hipStream_t)stream);
}

extern "C" int dd_sampler_reset_resample(const dd_sampler* s, const dd_resample* resample, void* stream) {
  if (!s || !resample || resample->size < (int32_t)sizeof(dd_resample) || !resample->epoch) return DD_ERR_BAD_ARG;
  int rc = dd_sampler_reset(s, stream);
  if (rc != DD_OK) return rc;
  return dd::launch_reset_epoch(resample->epoch, (hipStream_t)stream);
}

static int graph_create_impl(const dd_sampler* s, const dd_model_opts* opts, const uint64_t* sample_keys, const dd_fixed* fixed,
                             const dd_resample* rsm, const dd_restraints* rst, int steps_per_graph, void* stream, void** graph_out) {
  hipStream_t st = (hipStream_t)stream;
  dd::ModelOpts mo;
  dd::StepExtras x;
  if (!graph_out || steps_per_graph < 1 || steps_per_graph > 64) return DD_ERR_BAD_ARG;
  int rc = read_step_extras(s, opts, sample_keys, fixed, rsm, rst, st, true, &mo, &x);
  if (rc != DD_OK) return rc;
  StepGraph* g = new StepGraph();
  rc = capture_steps(s, mo, x, steps_per_graph, st, &g->graph, &g->exec);
  if (rc != DD_OK) {
    delete g;
    return rc;
  }
  *graph_out = g;
  return DD_OK;
}

extern "C" int dd_graph_launch(void* graph, int n_graphs, void* stream) {
  StepGraph* g = (StepGraph*)graph;
  if (!g || g->magic != 0x44444753u || !g->exec || n_graphs < 0 || !stream) return DD_ERR_BAD_ARG;
  for (int i = 0; i < n_graphs; ++i)
    if (hipGraphLaunch(g->exec, (hipStream_t)stream) != hipSuccess) { (void)hipGetLastError(); return DD_ERR_HIP; }
  return DD_OK;
}

extern "C" int dd_graph_destroy(void* graph) {
  StepGraph* g = (StepGraph*)graph;
  if (!g || g->magic != 0x44444753u) return DD_ERR_BAD_ARG;
  g->magic = 0;
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (g->graph) (void)hipGraphDestroy(g->graph);
  delete g;
  return DD_OK;
}

extern "C" int dd_sample_steps_graph_multi(const dd_sampler* const* ss, int n, int n_steps, void* const* streams) {
  return dd_sample_steps_graph_multi_ex(ss, nullptr, n, n_steps, streams);
}

extern "C" int dd_sample_steps_graph_multi_ex(const dd_sampler* const* ss, const dd_bond_head* const* bhs, int n, int n_steps,
                                              void* const* streams) {
  return dd_sample_steps_graph_multi_ex2(ss, bhs, nullptr, n, n_steps, streams);
}

extern "C" int dd_sample_steps_graph_multi_ex2(const dd_sampler* const* ss, const dd_bond_head* const* bhs, const dd_node_out* const* nos,
                                               int n, int n_steps, void* const* streams) {
  if (n <= 0 || n > 64) return DD_ERR_BAD_ARG;
  dd_model_opts o[64];
  const dd_model_opts* po[64];
  for (int i = 0; i < n; ++i) {
    o[i] = opts_of(bhs ? bhs[i] : nullptr, nos ? nos[i] : nullptr);
    po[i] = &o[i];
  }
  return dd_sample_steps_graph_multi_opts(ss, po, n, n_steps, streams);
}

extern "C" int dd_sample_steps_graph_multi_opts(const dd_sampler* const* ss, const dd_model_opts* const* opts, int n, int n_steps,
                                                void* const* streams) {
  if (!ss || !streams || n <= 0 || n > 64 || n_steps < 0) return DD_ERR_BAD_ARG;
  dd::ModelOpts mos[64];
  for (int i = 0; i < n; ++i) {
    if (read_model_opts(opts ? opts[i] : nullptr, &mos[i]) != DD_OK || !ss[i] || check_model(ss[i], mos[i]) == DD_ERR_BAD_ARG) return DD_ERR_BAD_ARG;
    const dd_sampler* s = ss[i];
    if (!check_step_sampler(s) || !streams[i]) return DD_ERR_BAD_ARG;
    for (int j = 0; j < i; ++j)
      if (streams[j] == streams[i] || ss[j]->workspace == s->workspace) return DD_ERR_BAD_ARG;
    int rc = dd::check_shapes(s);
    if (rc != DD_OK) return rc;
  }
  if (n_steps == 0) return DD_OK;
  hipGraph_t graph[64] = {};
  hipGraphExec_t exec[64] = {};
  int rc = DD_OK;
  // the side streams / events used inside a step are shared, which is fine: they only shape each graph while it
  // is being captured, one chain at a time; the replays below do not touch them
  for (int i = 0; i < n && rc == DD_OK; ++i)
    rc = capture_steps(ss[i], mos[i], dd::StepExtras(), 1, (hipStream_t)streams[i], &graph[i], &exec[i]);
  if (rc == DD_OK) {
    static const int threaded = [] { const char* e = getenv("DD_MULTI_THREADS"); return e ? atoi(e) : 1; }();
    if (threaded) {
      // one host thread per chain: replaying a graph of ~60 kernel nodes costs the host about as much time as a small
      // chain takes on the GPU, so a single launching thread would be the bottleneck
      int dev = 0;
      (void)hipGetDevice(&dev);
      std::vector<std::thread> th;
      std::vector<int> trc(n, DD_OK);
      for (int i = 0; i < n; ++i)
        th.emplace_back([&, i] {
          if (hipSetDevice(dev) != hipSuccess) { trc[i] = DD_ERR_HIP; return; }
          for (int k = 0; k < n_steps; ++k)
            if (hipGraphLaunch(exec[i], (hipStream_t)streams[i]) != hipSuccess) { trc[i] = DD_ERR_HIP; return; }
        });
      for (auto& t : th) t.join();
      for (int i = 0; i < n; ++i) if (trc[i] != DD_OK) rc = trc[i];
    } else {
      for (int k = 0; k < n_steps && rc == DD_OK; ++k)
        for (int i = 0; i < n; ++i)
          if (hipGraphLaunch(exec[i], (hipStream_t)streams[i]) != hipSuccess) { rc = DD_ERR_HIP; break; }
    }
  }
  for (int i = 0; i < n; ++i)
    if (hipStreamSynchronize((hipStream_t)streams[i]) != hipSuccess) rc = rc == DD_OK ? DD_ERR_HIP : rc;
  for (int i = n - 1; i >= 0; --i) {                      // newest first (see model.py::_evict_chain_cache)
    if (exec[i]) (void)hipGraphExecDestroy(exec[i]);
    if (graph[i]) (void)hipGraphDestroy(graph[i]);
  }
  if (rc != DD_OK) (void)hipGetLastError();
  return rc;
}

extern "C" int dd_profile_step(const dd_sampler* s, int n_iters, float* ms_per_category, void* stream) {
  if (!s || !ms_per_category || n_iters <= 0) return DD_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  static dd::Profiler prof;
  if (!prof.created) {
    for (int i = 0; i < dd::Profiler::MAXEV; ++i) {
      if (hipEventCreate(&prof.start[i]) != hipSuccess || hipEventCreate(&prof.stop[i]) != hipSuccess) return DD_ERR_HIP;
    }
    prof.created = 1;
  }
  for (int c = 0; c < DD_NUM_PROF_CATS; ++c) ms_per_category[c] = 0.f;
  int rc = DD_OK;
  for (int it = 0; it < n_iters && rc == DD_OK; ++it) {
    prof.n = 0;
    dd::g_prof = &prof;
    rc = one_step(s, st);
    { dd::ProfScope empty_pair(DD_PROF_EVENT_PAIR, st); }
    dd::g_prof = nullptr;
    if (hipStreamSynchronize(st) != hipSuccess) return DD_ERR_HIP;
    for (int i = 0; i < prof.n; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, prof.start[i], prof.stop[i]) != hipSuccess) return DD_ERR_HIP;
      ms_per_category[prof.cat[i]] += ms;
    }
  }
  for (int c = 0; c < DD_NUM_PROF_CATS; ++c) ms_per_category[c] /= (float)n_iters;
  return rc;
}

// Profiling aid: when set, the tiled attention kernel of class `mode` (0 NE,1 NB,2 BL,3 PE,4 PB) writes 16
// s_memtime stamps per workgroup (wave 0) into `buf` ([n_workgroups][16] int64, device memory).
static int g_options_epoch = 0;
extern "C" int dd_debug_set_clock_buffer(long long* buf, int mode) {
  ++g_options_epoch;
  if (mode == 100) { dd::g_gemm_dbg = buf; return DD_OK; }      // dd_gemm128 phase stamps
  if (mode == 200) { dd::g_node_trace = buf; return DD_OK; }    // per-workgroup clocks of the fused node launch (-DDD_NODE_TRACE=1 builds)
  dd::g_gemm_dbg = nullptr;
  dd::g_dbg_clock = buf;
  dd::g_dbg_mode = buf ? mode : -1;
  return DD_OK;
}

// Profiling aid: 0 = one launch per sub-layer (so dd_profile_step can time each kernel class), 1 = fused launches.
// Bumped by every dd_debug_set_* call: hosts that keep captured step graphs (model.py's chain cache) compare it to know
// when the launch structure may have changed under them.
extern "C" int dd_debug_options_epoch(void) { return g_options_epoch; }

extern "C" int dd_debug_set_fusion(int mode) {
  ++g_options_epoch;
  if (mode != 0 && mode != 1 && mode != 3) return DD_ERR_BAD_ARG;
  dd::g_fuse = (mode == 1 || mode == 3) ? 1 : 0;
  dd::g_overlap = mode == 1 ? 1 : 0;
  return DD_OK;
}

namespace dd { extern int g_pos_g_mode; extern int g_gemm_ksplit; extern int g_attn_waves; extern int g_attn_persist; extern int g_pos_waves; extern int g_bl_first; extern int g_gemm_xcd; }
// Measurement aid: runtime switches for A/B timing inside one process.  key 0: attention launch structure (same
// values as dd_debug_set_fusion), key 1: K-split projection GEMM tiles (1 = on).
// First bounded spin of the layer-tail hand-offs that gave up (0 = none) since the word was last read (sticky; the
// workspace must be zero-initialised once): 100+j / 200+j a queue tile of job j, 300/301 assemble, 400 coordinate attention, 500 node attention.
// Synchronises the stream.  A non-zero code means the launches did not overlap as the schedule assumes (results invalid).
#if defined(DD_DEBUG_OPTIONS) && DD_DEBUG_OPTIONS          // (the default library has no polling schedule: not exported there)
extern "C" int dd_queue_error(const dd_sampler* s, void* stream, int* code) {
  if (!s || !s->workspace || !code) return DD_ERR_BAD_ARG;
  dd::Workspace w = dd::carve(s->workspace, s->B, s->NP, s->NL, s->K);
  int32_t v = 0;
  if (hipMemcpyAsync(&v, w.counters + dd::DD_NUM_COUNTERS + dd::DD_FLAG_ERR, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return DD_ERR_HIP;
  *code = (int)v;
  if (v != 0 && hipMemsetAsync(w.counters + dd::DD_NUM_COUNTERS + dd::DD_FLAG_ERR, 0, sizeof(v), (hipStream_t)stream) != hipSuccess) return DD_ERR_HIP;
  return DD_OK;
}
#endif

extern "C" int dd_debug_node_split(int B, int NP, int NL, int K) { return dd::node_split_lookup(B, NP, NL, K); }

// bit 0: the projections of the new h (and the heads' first Linear) run inside the coordinate launch (k_attn2_pos_g), not as a GEMM launch
extern "C" int dd_debug_schedule(void) { return dd::g_p2_in_pos ? 1 : 0; }

extern "C" int dd_debug_set_option(int key, int value) {
  ++g_options_epoch;
  if (key == 0) return dd_debug_set_fusion(value);
#if defined(DD_DEBUG_OPTIONS) && DD_DEBUG_OPTIONS
  if (key == 1) { dd::g_gemm_ksplit = value ? 1 : 0; return DD_OK; }
  if (key == 3) { dd::g_attn_persist = value ? 1 : 0; return DD_OK; }
  if (key == 24) { dd::g_head_fused = value ? 1 : 0; return DD_OK; }
  if (key == 22) { dd::g_l0_tables = value ? 1 : 0; return DD_OK; }
  if (key == 21) { dd::g_gemm_xcd = value ? 1 : 0; return DD_OK; }
  if (key == 20) { dd::g_step_fold = value ? 1 : 0; return DD_OK; }
  if (key == 19) { dd::g_xup_in_asm = value ? 1 : 0; return DD_OK; }
  if (key == 18) { if (value < 0 || value > 1024) return DD_ERR_BAD_ARG; dd::g_bl_first = value; return DD_OK; }
  if (key == 17) { dd::g_pb_early = value ? 1 : 0; return DD_OK; }
  if (key == 16) { dd::g_lin_with_pb2 = value ? 1 : 0; return DD_OK; }
  if (key == 14) { dd::g_defer_pos = value ? 1 : 0; return DD_OK; }
  if (key == 13) { dd::g_fused_max_nl = value; return DD_OK; }
  if (key == 12) { dd::g_q1_in_gemm = value ? 1 : 0; return DD_OK; }
  if (key == 11) { dd::g_xup_in_pos = value ? 1 : 0; return DD_OK; }
  if (key == 9) { dd::g_q_in_pos = value ? 1 : 0; return DD_OK; }
  if (key == 8) { if (value < 0 || value > 5) return DD_ERR_BAD_ARG; dd::g_sched = value; return DD_OK; }
  if (key == 25) { dd::g_tail_variant = value; return DD_OK; }
  if (key == 27) { dd::g_side_lin = value ? 1 : 0; return DD_OK; }
  if (key == 30) { dd::g_p2_in_pos = value ? 1 : 0; return DD_OK; }
  if (key == 31) { dd::g_pos_g_mode = value & 3; return DD_OK; }
  if (key == 28) { dd::g_heads_early = value ? 1 : 0; return DD_OK; }
  if (key == 32) { dd::g_lin_in_node = value < 0 ? -1 : (value ? 1 : 0); return DD_OK; }
  if (key == 29) { dd::g_head_rows_first = value ? 1 : 0; return DD_OK; }
  if (key == 7) { dd::g_step_fused = value ? 1 : 0; return DD_OK; }
  if (key == 5) { if (value != 2 && value != 4 && value != 8) return DD_ERR_BAD_ARG; dd::g_pos_waves = value; return DD_OK; }
  if (key == 2) { if (value != 8) return DD_ERR_BAD_ARG; dd::g_attn_waves = value; return DD_OK; }
  return DD_ERR_BAD_ARG;
#else
  (void)value;
  return DD_ERR_BAD_ARG;                                 // (the alternatives live in the measurement build only)
#endif
}
