// Node output MLPs of a layer (x2h_out_fc: True; uni_transformer_edge.py:39-40, 70-71, 277) as ONE launch:
//
//   z_e   = relu(LN_e(W1_e [A_e ; h] + b1_e))            node_layer_with_edge.node_output
//   z_b   = relu(LN_b(W1_b [A_b ; h] + b1_b))            node_layer_with_bond.node_output (A_b = 0 on protein rows)
//   h_new = h + W2_e' z_e + W2_b' z_b + c0                W2_m' = W_lin W2_m,  c0 = W_lin (b2_e + b2_b) + b_lin
//
// (the lin_node products are composed on the host: packing.node_out_fc).  It takes the place of the lin_node GEMM of a layer.
//
// A workgroup of 256 threads owns 32 rows and all 128 columns -- the LayerNorm needs a row's 128 pre-activations in one place --
// wave w the columns 32 w .. 32 w + 31 (one 32 x 32 accumulator, v_mfma_f32_32x32x2_f32: exact fp32 fmaf chains like every other
// Linear here).  The six 128 x 128 weight images go through LDS in 64-wide K pieces (12 pieces of 128 x 64, pitch 66), the next
// piece's global loads in flight while the current one is multiplied, as the K-split tile of dd_gemm_tile.hpp does; the input
// rows go the same way (32 x 64, pitch 66).  The two hidden rows stay in LDS (2 x 32 x 128, pitch 130) and are the A operand of the
// second products.  LDS: (32 + 128) * 66 + 2 * 32 * 130 floats = 75.5 KB, two workgroups per CU.
// Workgroups without a ligand row skip the two pieces of U_b = W1_b[:, :128] (their A_b is zero).
#include "dd_kernels.hpp"

namespace dd {

constexpr int NO_ROWS = 32;
constexpr int NO_PH = 66;      // pitch of a K piece: (66 row) mod 64 = 2 row -> conflict-free ds_read_b64 operand fetches
constexpr int NO_PZ = 130;     // pitch of the hidden rows, likewise

__global__ __launch_bounds__(256) void k_node_out_fc(NodeOutArgs a) {
  __shared__ __attribute__((aligned(16))) float sm[(NO_ROWS + 128) * NO_PH + 2 * NO_ROWS * NO_PZ];
  float* Xh = sm;
  float* Wh = sm + NO_ROWS * NO_PH;
  float* Z = Wh + 128 * NO_PH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
  const int N = a.NP + a.NL;
  const long R = (long)a.B * N;
  const long row0 = (long)blockIdx.x * NO_ROWS;
  // first ligand row at or behind row0: inside this tile?
  bool has_lig;
  {
    const long b0 = row0 / N;
    const int n0 = (int)(row0 - b0 * N);
    const long first = n0 >= a.NP ? row0 : b0 * N + a.NP;
    has_lig = first < row0 + NO_ROWS && first < R;
  }
  // pieces 0-3: W1_e over [A_e ; h], 4-7: W1_b over [A_b ; h], 8-9: W2_e' over z_e, 10-11: W2_b' over z_b
  auto next_piece = [&](int s) { return (s == 3 && !has_lig) ? 6 : s + 1; };
  float4 xv[2], wv[8];
  auto fetch = [&](int s) {
    const float* Wp;
    int ldw;
    if (s < 8) { Wp = a.blk + ((s >> 2) ? DD_NO_W1B : DD_NO_W1E) + (s & 3) * 64; ldw = 256; }
    else { Wp = a.blk + (((s - 8) >> 1) ? DD_NO_W2B : DD_NO_W2E) + ((s - 8) & 1) * 64; ldw = 128; }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = tid + k * 256, r = i >> 4, c4 = (i & 15) * 4;
      wv[k] = *reinterpret_cast<const float4*>(Wp + (long)r * ldw + c4);
    }
    if (s >= 8) return;
    const int q = s & 3;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = tid + k * 256, r = i >> 4, c4 = (i & 15) * 4;
      const long gr = row0 + r;
      const float* src = nullptr;
      if (gr < R) {
        if (q >= 2) src = a.h + gr * 128 + (q - 2) * 64 + c4;
        else if (s < 4) src = a.Ae + gr * 128 + q * 64 + c4;
        else {
          const long b = gr / N;
          const int n = (int)(gr - b * N);
          if (n >= a.NP) src = a.Ab + (b * a.NL + (n - a.NP)) * 128 + q * 64 + c4;
        }
      }
      xv[k] = src ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto commit = [&](int s) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = tid + k * 256, r = i >> 4, c4 = (i & 15) * 4;
      float2* e = reinterpret_cast<float2*>(&Wh[r * NO_PH + c4]);
      e[0] = make_float2(wv[k].x, wv[k].y);
      e[1] = make_float2(wv[k].z, wv[k].w);
    }
    if (s >= 8) return;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = tid + k * 256, r = i >> 4, c4 = (i & 15) * 4;
      float2* d = reinterpret_cast<float2*>(&Xh[r * NO_PH + c4]);
      d[0] = make_float2(xv[k].x, xv[k].y);
      d[1] = make_float2(xv[k].z, xv[k].w);
    }
  };
  // LayerNorm + ReLU of hidden row m in place: 8 threads per row, 16 channels each; the channels are added pairwise (in the
  // thread, then a 3-step butterfly), so a constant row has mean = its value exactly and comes out as relu(beta)
  auto ln_relu = [&](int m) {
    const int row = tid >> 3, seg = tid & 7;
    float* p = Z + (m * NO_ROWS + row) * NO_PZ + seg * 16;
    const float* ln = a.blk + (m ? DD_NO_LNB : DD_NO_LNE) + seg * 16;
    float v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float2 t = *reinterpret_cast<const float2*>(p + 2 * i);
      v[2 * i] = t.x; v[2 * i + 1] = t.y;
    }
    auto tree16 = [](const float (&u)[16]) {
      return (((u[0] + u[1]) + (u[2] + u[3])) + ((u[4] + u[5]) + (u[6] + u[7]))) +
             (((u[8] + u[9]) + (u[10] + u[11])) + ((u[12] + u[13]) + (u[14] + u[15])));
    };
    auto oct_sum = [](float s) {
      s += dpp_mov<0xB1>(s); s += dpp_mov<0x4E>(s); s += dpp_mov<0x141>(s);
      return s;
    };
    const float mean = oct_sum(tree16(v)) * (1.0f / 128.0f);
    float d2[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { v[i] -= mean; d2[i] = v[i] * v[i]; }
    const float rstd = dd_rsqrt(oct_sum(tree16(d2)) * (1.0f / 128.0f) + 1e-5f);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float2 g = *reinterpret_cast<const float2*>(ln + 2 * i), be = *reinterpret_cast<const float2*>(ln + 128 + 2 * i);
      *reinterpret_cast<float2*>(p + 2 * i) = make_float2(fmaxf(fmaf(v[2 * i] * rstd, g.x, be.x), 0.f),
                                                         fmaxf(fmaf(v[2 * i + 1] * rstd, g.y, be.y), 0.f));
    }
  };

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int col = wave * 32 + li;
  const float* wb = &Wh[col * NO_PH + 2 * hh];
  int s = 0;
  fetch(0);
  for (;;) {
    __syncthreads();                                     // the previous piece's operand reads (and the hidden rows' writes) are done
    commit(s);
    __syncthreads();
    const int nx = next_piece(s);
    if (nx < 12) fetch(nx);
    const float* xa = s < 8 ? &Xh[li * NO_PH + 2 * hh] : &Z[(((s - 8) >> 1) * NO_ROWS + li) * NO_PZ + ((s - 8) & 1) * 64 + 2 * hh];
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const float2 av = *reinterpret_cast<const float2*>(xa + 4 * kk);
      const float2 bv = *reinterpret_cast<const float2*>(wb + 4 * kk);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
    }
    if (s == 3 || s == 7) {                              // pre-activations of MLP m complete: + b1 -> hidden row buffer
      const int m = s >> 2;
      const float b1 = a.blk[(m ? DD_NO_B1B : DD_NO_B1E) + col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;   // C/D map: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        Z[(m * NO_ROWS + row) * NO_PZ + col] = acc[r] + b1;
        acc[r] = 0.f;
      }
      if (s == 7) {
        __syncthreads();
        ln_relu(0);
        ln_relu(1);
      }
    }
    if (nx >= 12) break;
    s = nx;
  }
  // h_new = h + (acc + c0): 128 contiguous bytes per half wave and register
  const float c0 = a.blk[DD_NO_C0 + col];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long gr = row0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
    if (gr < R) a.out[gr * 128 + col] = a.h[gr * 128 + col] + (acc[r] + c0);
  }
}

int launch_node_out_fc(const NodeOutArgs& a, hipStream_t st) {
  const long R = (long)a.B * (a.NP + a.NL);
  if (R <= 0) return DD_OK;
  hipLaunchKernelGGL(k_node_out_fc, dim3((unsigned)((R + NO_ROWS - 1) / NO_ROWS)), dim3(256), 0, st, a);
  DD_CHECK_LAUNCH();
  return DD_OK;
}

}  // namespace dd

extern "C" int dd_node_out_fc(const float* A_e, const float* A_b, const float* h, int B, int NP, int NL, const float* weights,
                              const int32_t* np_real, const int32_t* nl_real, float* h_out, void* stream) {
  if (!A_e || !A_b || !h || !weights || !h_out || B <= 0 || NP < 0 || NL <= 0) return DD_ERR_BAD_ARG;
  if (((reinterpret_cast<size_t>(A_e) | reinterpret_cast<size_t>(A_b) | reinterpret_cast<size_t>(h) | reinterpret_cast<size_t>(weights) |
        reinterpret_cast<size_t>(h_out)) & 15) != 0)
    return DD_ERR_BAD_ARG;
  (void)np_real; (void)nl_real;                          // padding rows are computed like real ones (as the lin_node GEMM does)
  dd::NodeOutArgs a{A_e, A_b, h, h_out, weights, B, NP, NL};
  return dd::launch_node_out_fc(a, (hipStream_t)stream);
}
