// kh_model_gemm.hip — everything that runs on the GEMM slabs (kh_gemm.h, kh_pattn.h): ONE layer driver, launch_pg_pass,
// and ONE GEMM launch, pg_gemm, under the three calls that differ only in where a slab token sits - the fp32-MFMA
// prompt prefill (kh_model_prefill_gemm: a run of positions), the prefill into sequence slots (kh_seq_prefill.h: a
// tile table; kh_model_seq.hip checks the call and drives it) and the wide sequence pass (kh_seq_gemm.h: a lane table
// at full depth; what kh_model_seq_step_gemm and kh_model_generate_batch_gemm enqueue) - with their slabs, the launch
// plan of one GEMM (pg_shape, pg_plan) and the operator-level entry of the MFMA slice attention.  Reads fp32 or int8
// weights - and, under KH_FLAG_GEMM16, the 16-bit copy on the bf16 matrix cores (pg_gemm; the kernels are compiled in
// kh_model_gemm_w16.hip).  The reference feeds the prompt one token per forward pass
// (demo/main.cpp:20-22) and decodes one sequence per process (demo/main.cpp:16-50).
// gfx950 only.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "kh_dispatch.h"
#include "kh_gemm.h"
#include "kh_model_internal.h"
#include "kh_pattn.h"
#include "kh_seq_gemm.h"
#include "kh_seq_prefill.h"

using namespace khm;

bool khm::pg_supported(const kh_model* m) {
  const kh_config& c = m->cfg;
  if (c.head_size <= 32) return false;  // attention: the fast multi-token decode kernel
  const int kq = c.is_quant ? 64 : 16;  // K granule of one MFMA operand load
  if (c.dim % kq || c.hidden_dim % kq || c.dim % 16 || c.kv_dim % 16 || c.hidden_dim % 16) return false;
  if (c.is_quant && m->gshift != 6) return false;
  return true;
}

namespace {
// slabs of KH_PG_TMAX token rows
int ensure_pg_buffers(kh_model* m) {
  if (m->pg_x) return KH_OK;
  const kh_config& c = m->cfg;
  const size_t T = KH_PG_TMAX;
  int rc;
  auto zalloc = [&](KhDev<float>& b, size_t n) -> int {
    if ((rc = b.alloc(n)) != KH_OK) return rc;
    // rows beyond the valid tokens are read as MFMA operands (their columns are discarded):
    // they must hold finite numbers
    return (int)hipMemsetAsync(b, 0, n * sizeof(float), m->stream);
  };
  // a failure half-way leaves the model without any slab: a later call starts over
  KhDev<float> x, xn, q, att, h, part;
  if ((rc = zalloc(x, T * c.dim)) != KH_OK || (rc = zalloc(xn, T * c.dim)) != KH_OK ||
      (rc = zalloc(q, T * c.dim)) != KH_OK || (rc = zalloc(att, T * c.dim)) != KH_OK ||
      (rc = zalloc(h, T * c.hidden_dim)) != KH_OK ||
      (rc = zalloc(part, (size_t)KH_PG_KZ_MAX * T * c.dim)) != KH_OK)  // K-slice partial rows
    return rc;
  m->pg_x = std::move(x);
  m->pg_xn = std::move(xn);
  m->pg_q = std::move(q);
  m->pg_att = std::move(att);
  m->pg_h = std::move(h);
  m->pg_part = std::move(part);
  return KH_OK;
}
// does the prompt-slice attention run on the MFMA kernel (kh_pattn.h)?  KH_PG_ATTN=0 forces the fallback.
bool pg_mfma_attn(const kh_model* m) { return !dbg_off("KH_PG_ATTN") && pg_attn_supported(m->cfg.head_size); }
// The split workspace of the decode-attention FALLBACK (one per token of a pass, ~270 KB per token at
// Llama-3.2-1B geometry: 136 MB for a 512-token pass).  Every BASELINE head size has an MFMA
// instantiation, so it is allocated on the first pass that actually takes the fallback.
int ensure_pg_ws(kh_model* m) {
  if (m->pg_ws || pg_mfma_attn(m)) return KH_OK;
  m->pg_ws_tok_bytes = (attn_ws_bytes(m->cfg.head_num, m->cfg.head_size, m->attn_ws_stride) + 255) & ~(size_t)255;
  if (!m->pg_ws_tok_bytes) return KH_OK;
  KhDev<char> ws;
  int rc;
  if ((rc = ws.alloc(m->pg_ws_tok_bytes * (size_t)KH_PG_TMAX)) != KH_OK) return rc;
  KH_CHECK_HIP(hipMemsetAsync(ws, 0, m->pg_ws_tok_bytes * (size_t)KH_PG_TMAX, m->stream));
  m->pg_ws = std::move(ws);
  return KH_OK;
}
}  // namespace
int khm::prefill_gemm_prepare(kh_model* m) {
  const int rc = ensure_pg_buffers(m);
  return rc == KH_OK ? ensure_pg_ws(m) : rc;
}

namespace {
// the (R, NT) register tiles k_pg_gemm is compiled for, and the waves per SIMD that fit with each
constexpr int kPgTiles[4][3] = {{2, 8, 2}, {2, 4, 3}, {2, 2, 4}, {1, 4, 4}};
constexpr int pg_tile(int R, int NT) {  // index in kPgTiles, -1: no such tile
  for (int i = 0; i < 4; ++i)
    if (kPgTiles[i][0] == R && kPgTiles[i][1] == NT) return i;
  return -1;
}
struct PgShape {
  int R, NT, ks, slices;
  bool solo;
  int kz;
};
// Launch shape of one prefill GEMM (kh_gemm.h): R 16-row tiles and NT 16-token tiles per wave,
// ks waves splitting K per workgroup, grid.y token slices.  Picked by a small cost model of the
// busiest SIMD, fitted to a sweep on Llama-3.2-1B (profiles/r2_gemm_shape_sweep.txt):
//   * a workgroup lives on ONE CU: fewer than 256 workgroups leave CUs idle (the model prices the
//     busiest CU, so such shapes simply show their long per-wave work);
//   * fp32: ONE wave per SIMD is the sweet spot: two MFMA-bound waves on a SIMD cost ~1.6x the
//     time of the same work in one wave (the (w1,w3) GEMM went 140 -> 84 us per launch from 8 to 4
//     waves per CU), three or more ~1.8x;  int8: the opposite - its waves spend VALU time on the
//     dequant between MFMAs, so a second and third wave per SIMD fill the matrix pipe
//     (profiles/r2_gemm_shape_sweep_7b.txt: (w1,w3) 2 -> 4 waves per workgroup 30.4 -> 23.3 ms per
//     prefill), up to what the register file admits;
//     (these penalties were fitted with the phase scheme in every fp32 loop; since the uniform
//     operand rings of kh_gemm.h a second wave per SIMD costs less - (w1,w3) with 8 instead of 4
//     waves per workgroup: 3.01 vs 2.75 ms per 128-token pass - but still loses, and a re-sweep of
//     13 forced shapes leaves every choice of the model in place, profiles/r3_prefill_shapes512.txt);
//   * bigger register tiles need fewer operand bytes per MFMA (small factor), more token slices
//     re-read the weights from L2 (small factor), padding tokens are wasted MFMAs;
//   * fp32 passes of more than 128 tokens launch several times 256 workgroups, which would sit two
//     or more to a CU - two or more MFMA-bound waves per SIMD.  `solo` keeps ONE workgroup per CU at
//     a time (a dynamic-LDS request above half the CU's 160 KiB; the workgroups of a CU then run back
//     to back at the one-wave-per-SIMD rate) and is priced as such: Llama-3.2-1B, 512-token pass,
//     56.4 k prompt tok/s with it, 38.0 k without (profiles/r3_prefill_wide.txt).  Passes of <= 128
//     tokens use it for the MFMA-bound (2,8) tile only (Llama-2-7B fp32: 344 / 384 workgroups); their
//     small latency-bound tiles gain from a partner wave, and whole rounds of 256 cost more than
//     they save (Qwen2.5, (1,4) tile in 608 workgroups: 45.9 k shared, 41.8 k solo).
//   * the residual GEMMs (wo, w2) may split K across `kz` workgroups as well (blockIdx.z): with 2048
//     rows x 128 tokens there are only 64 (2,8) tiles, so a chip-filling launch either takes small
//     tiles or more K slices than a workgroup has waves.  The slices store partial rows and the
//     RMSNorm kernel that follows adds them in fixed order (kh_gemm.h) - no ticket, no second launch.
// hooks read per call (kh_debug_set takes effect on the next launch plan)
inline bool pg_solo_on() { return !dbg_off("KH_PG_SOLO"); }
inline bool pg_kz_on() { return !dbg_off("KH_PG_KZ"); }
//   * the loop on the 16-bit copy (kh_gemm_w16.h; allow_solo = false) spends VALU time on the activation split between
//     its MFMAs, so - like int8 - it gains from a partner wave on the SIMD and `solo` only costs: 512-token prefill with
//     KH_PG_SOLO=0 against the default, Llama-3.2-1B 6.14 vs 6.32 ms, Llama-2-7B 39.4 vs 41.1 ms, Qwen2.5-0.5B 4.82 vs
//     6.29 ms (profiles/gemm16_shape_sweep.txt).  Everything else of the model is the fp32 fit, unchanged.
//   * the int8 loop on the bf16 matrix cores (kh_gemm_q16.h; tile28 = false) has no (2,8) register tile: the model picks
//     among the other three, with the int8 fit otherwise unchanged.
PgShape pg_shape(int T, int rows_total, bool r2_ok, int nm, int kblocks, int min_blocks, bool quant, bool allow_kz,
                 bool allow_solo = true, bool tile28 = true) {
  const int nt_all = (T + 15) / 16;
  const bool wide = nt_all > 8;  // a pass of more than 128 tokens
  PgShape best{1, 4, 1, (nt_all + 3) / 4, false, 1};
  double best_cost = -1.0;
  for (const auto& c : kPgTiles) {
    const int R = c[0], NT = c[1], occ = c[2];
    if (R == 2 && !r2_ok) continue;
    if (R == 1 && quant && r2_ok) continue;  // int8: the 32-row tile measured better wherever it fits
    if (NT > 4 && (nt_all <= 4 || !tile28)) continue;  // no 128-token tile for <= 64 tokens
    const int slices = (nt_all + NT - 1) / NT;
    for (int kz = 1; kz <= (allow_kz && pg_kz_on() ? KH_PG_KZ_MAX : 1); kz *= 2)
    for (int ks = 1; ks * nm * 64 <= KH_PG_WG_MAX(quant); ks *= 2) {
      const long wgs = (long)(rows_total / (16 * R)) * slices * kz;
      if (ks * kz > 1 && kblocks / (ks * kz) < min_blocks) break;  // keep a useful K range per wave
      // waves per SIMD on the busiest CU.  A workgroup counts as one wave on EACH SIMD it touches:
      // two 2-wave workgroups on a CU were measured on the same two SIMDs (Llama-3.2-1B, 256 tokens:
      // the (2,8) SwiGLU tile with 2-wave workgroups 255 us against 2 x 83 us for two 128-token
      // launches of 4-wave workgroups)
      const long cu_wgs = (wgs + 255) / 256;
      long wps = cu_wgs * ((nm * ks + 3) / 4);
      const long rounds = (wps + occ - 1) / occ;                    // beyond the register file: queued
      if (wps > occ) wps = occ;
      const double pen = quant ? (wps <= 1 ? 1.0 : (wps == 2 ? 0.72 : 0.62))
                               : (wps <= 1 ? 1.0 : (wps == 2 ? 1.6 : 1.8));
      const double per_wave = (double)((kblocks + ks * kz - 1) / (ks * kz)) * R * NT;
      double cost = per_wave * (double)(wps * rounds) * pen;
      cost *= 1.0 + 0.04 * (double)(kz - 1);  // partial rows written, and read back by the RMSNorm
      cost *= 1.0 + 0.15 * (double)(R + NT) / (double)(R * NT);
      // every token slice re-reads the weights from L2 - and, int8, dequantises them again
      cost *= 1.0 + (quant ? 0.15 : 0.05) * (double)(slices - 1);
      cost *= (double)(slices * NT) / (double)nt_all;
      bool solo = false;
      if (allow_solo && !quant && (wide || R * NT >= 16) && pg_solo_on() && wgs > 256) {
        const long wg_wps = (nm * ks + 3) / 4;
        const double c1 = per_wave * (double)(((wgs + 255) / 256) * wg_wps) * (wg_wps <= 1 ? 1.0 : (wg_wps == 2 ? 1.6 : 1.8));
        if (c1 < per_wave * (double)(wps * rounds) * pen) {
          cost *= c1 / (per_wave * (double)(wps * rounds) * pen);
          solo = true;
        }
      }
      if (best_cost < 0 || cost < best_cost) {
        best_cost = cost;
        best = PgShape{R, NT, ks, slices, solo, kz};
      }
    }
  }
  return best;
}
}  // namespace
bool khm::pg_lds_opt_in(const void* kern, size_t lds) {
  if (lds > 48 * 1024) {
    // the >48 KiB dynamic-LDS opt-in is per (device, kernel): set once, not on every launch of
    // the prefill hot path; a refusal is reported here, not as a generic launch error later
    struct Done { int dev; const void* fn; size_t lds; };
    static thread_local std::vector<Done> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    bool hit = false;
    for (const auto& d : done) hit = hit || (d.dev == dev && d.fn == kern && d.lds >= lds);
    if (!hit) {
      if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return false;
      }
      done.push_back({dev, kern, lds});
    }
  }
  return true;
}
namespace {
// The launch shape of one GEMM of a pass: the cost model, the KH_PG_SHAPE_<QKV|RESID|SWIGLU|STORE> hook, KH_PG_DEBUG.
// epi: KH_PG_*; STORE (the classifier GEMM of the wide sequence pass) plans as a residual GEMM without a K split
// across workgroups.
// kcols: the columns of a K block of the loop that runs - 16 fp32, 64 int8, 32 on the 16-bit copy (kh_gemm_w16.h)
// q16: the int8 loop on the bf16 matrix cores runs (kh_gemm_q16.h): no (2,8) tile - a hook that asks for it gets (2,4)
PgShape pg_plan(const kh_model* m, int EPI, int T, int rows_total, bool r2_ok, int K, int kcols, bool q16 = false) {
  const bool q = m->cfg.is_quant;
  const int nm = EPI == KH_PG_SWIGLU ? 2 : 1;
  const bool w16 = kcols == 32;
  // (min_blocks: the same 256 columns per wave as fp32's 16 blocks of 16)
  PgShape sh = pg_shape(T, rows_total, r2_ok, nm, K / kcols, q ? 4 : (w16 ? 8 : 16), q, EPI == KH_PG_RESID, !w16 && !q16,
                           !q16);
  {  // tuning hook: KH_PG_SHAPE_<QKV|RESID|SWIGLU|STORE>="R,NT,ks[,kz]" overrides the heuristic
    static const char* const names[4] = {"KH_PG_SHAPE_QKV", "KH_PG_SHAPE_RESID", "KH_PG_SHAPE_SWIGLU",
                                         "KH_PG_SHAPE_STORE"};
    const char* const ov = dbg(names[EPI]);
    if (ov) {
      int R = 0, NT = 0, ks = 0, kz = 1;
      if (sscanf(ov, "%d,%d,%d,%d", &R, &NT, &ks, &kz) >= 3 && pg_tile(R, NT) >= 0 && (R != 2 || r2_ok) &&
          (ks == 1 || ks == 2 || ks == 4 || ks == 8) && ks * nm * 64 <= KH_PG_WG_MAX(q) &&
          (kz == 1 || (EPI == KH_PG_RESID && (kz == 2 || kz == 4))))
      {
        if (q16 && NT > 4) NT = 4;
        const int slices = ((T + 15) / 16 + NT - 1) / NT;
        sh = PgShape{R, NT, ks, slices,
                     !q && !w16 && (T > 128 || R * NT >= 16) && pg_solo_on() &&
                         (long)(rows_total / (16 * R)) * slices * kz > 256, kz};
      } else {
        // not a launch this GEMM has (e.g. R = 2 where 32 rows do not divide the matrices): say so rather than
        // let a test believe it forced a shape
        fprintf(stderr, "[kh] %s=\"%s\" rejected (R,NT 1,4%s, ks 1/2/4/8 up to %d waves%s): heuristic shape\n",
                names[EPI], ov, r2_ok ? " or 2,2/4/8" : "", KH_PG_WG_MAX(q) / 64 / nm,
                EPI == KH_PG_RESID ? ", kz 1/2/4" : "");
      }
    }
  }
  if (dbg("KH_PG_DEBUG"))
    fprintf(stderr, "[pg] epi %d rows %d K %d T %d -> R %d NT %d slices %d ks %d kz %d (%d wgs x %d waves%s)\n", EPI,
            rows_total, K, T, sh.R, sh.NT, sh.slices, sh.ks, sh.kz, rows_total / (16 * sh.R) * sh.slices * sh.kz,
            nm * sh.ks, sh.solo ? ", solo" : "");
  return sh;
}

// One pass of T slab tokens through the GEMM kernels.  Where a slab token's id, its RoPE row and its cache row come
// from is the only thing the callers differ in (wo, the SwiGLU pair, w2 and the RMSNorm do not care where a token
// sits):
//   step                    a run (kh_model_prefill_gemm)      tiles (prefill into slots)   lanes (the wide pass)
//   token placement         pos0: slab token t is position     a KhRgTiles table            a KhWideLanes table
//                           and cache row pos0 + t
//   embedding               kh_embedding_f32_host of toks      the same                     k_sg_embed from d_seq_tok
//   QKV GEMM                k_pg_gemm                          k_rg_gemm                    k_sg_gemm
//   RoPE where the          k_pg_rope                          k_rg_rope                    k_sg_rope
//   epilogue cannot rotate
//   attention               k_pg_attn, else the decode         k_rg_attn (the caller        seq_attn_enqueue per group of
//                           kernel with pg_ws (KH_PG_ATTN=0,   checked: MFMA only)          KH_PF_BMAX lanes
//                           odd head sizes)
//   wo's B operand          tiled iff MFMA attention ran       tiled                        row-major
//   wo / SwiGLU / w2 GEMM   k_pg_gemm                          k_pg_gemm                    k_sg_gemm
//   tile list               kPgTiles                           kPgTiles                     no (2,8): NT > 4 runs as NT = 4
//                                                                                           with the slices recomputed
//   depth                   stops behind the last layer's      the same                     full depth: the final
//                           K/V rows                                                        k_pg_rmsnorm and the KH_PG_STORE
//                                                                                           GEMM into sg_logits (the caller's
//                                                                                           seq_tail_enqueue per group follows)
struct PgPass {
  int T;
  const int32_t* toks;  // host ids of the T slab tokens; null: the lanes feed d_seq_tok
  bool full_depth;
  int pos0;                  // a run; 0 under a table
  const KhRgTiles* tiles;    // a tile table, T = 16 x its tiles
  const KhWideLanes* lanes;  // a lane table, with the call's slots[n] the 8-lane groups are cut from (T = n)
  const int32_t* slots;
  int n;
};
PgPass pg_run(const int32_t* toks, int T, int pos0) { return PgPass{T, toks, false, pos0, nullptr, nullptr, nullptr, 0}; }
PgPass pg_tiles(const int32_t* toks, int T, const KhRgTiles& tiles) {
  return PgPass{T, toks, false, 0, &tiles, nullptr, nullptr, 0};
}
PgPass pg_lanes(const KhWideLanes& lanes, const int32_t* slots, int n) {
  return PgPass{n, nullptr, true, 0, nullptr, &lanes, slots, n};
}
// lanes [g * KH_PF_BMAX ..) of a wide pass as the 8-lane table the attention and the tail read; *ng: how many are valid
KhSeqLanes pg_lane_group(const kh_model* m, const PgPass& p, int g, int* ng) {
  KhSeqLanes l;
  *ng = p.n - g * KH_PF_BMAX < KH_PF_BMAX ? p.n - g * KH_PF_BMAX : KH_PF_BMAX;
  for (int b = 0; b < KH_PF_BMAX; ++b) {
    const int i = g * KH_PF_BMAX + (b < *ng ? b : *ng - 1);
    const KhSeqSlot& t = m->seq_tab[p.slots[i]];
    l.pos[b] = p.lanes->pos[i];
    l.row[b] = p.lanes->row[i];
    l.slot[b] = p.lanes->slot[i];
    l.pfx_len[b] = t.pfx;
    l.pfx_row0[b] = t.pfx > 0 ? m->seq_tab[t.parent].row0 : 0;
  }
  return l;
}
inline int pg_lane_groups(const PgPass& p) { return (p.n + KH_PF_BMAX - 1) / KH_PF_BMAX; }

// One GEMM of a pass in its planned shape.  Returns, QKV: whether the epilogue rotates q / k itself (else the pass's
// rope kernel has to follow); RESID: the number of K slices whose partial rows the next RMSNorm has to add (0 = the
// epilogue added itself).  ok: cleared where the LDS opt-in of the shape is refused - that launch is skipped.
// on16: the GEMM's launch class (KH_W16_*) and its matrices in the 16-bit copy.  Where the class runs on the bf16 matrix
// cores (KH_FLAG_GEMM16: gemm16_runs) the same shape - planned in blocks of 32 columns - launches the _w16 stem
// (kh_gemm_w16.h, compiled in kh_model_gemm_w16.hip) with the weight pointers swapped; everything else is untouched.
// An int8 group-64 model under KH_FLAG_GEMM16_Q8 (gemm16_q8_runs) launches the _q16 stem on the image's own pointers.
struct PgOn16 {
  int cls;
  const void* w[3];
};
template <int EPI>
int pg_gemm(kh_model* m, const PgPass& p, int rows_total, bool r2_ok, KhPgGemmArgs a, bool* ok, const PgOn16& on16) {
  const int nm = EPI == KH_PG_SWIGLU ? 2 : 1;
  const bool w16 = gemm16_runs(m, on16.cls);
  const bool q16 = gemm16_q8_runs(m, on16.cls);  // (an int8 model: never both)
  PgShape sh = pg_plan(m, EPI, a.T, rows_total, r2_ok, a.K, w16 ? 32 : (m->cfg.is_quant ? 64 : 16), q16);
  if (p.lanes && sh.NT > 4) {  // a hook asked for the 128-token tile
    sh.NT = 4;
    sh.slices = ((a.T + 15) / 16 + 3) / 4;
  }
  if (EPI == KH_PG_QKV && a.rope == KH_PG_ROPE_TILES && (sh.R != 2 || sh.NT > 4))
    a.rope = KH_PG_ROPE_OFF;  // no partner tile in the wave / no registers to hold it: the rope kernel follows
  const int wg = nm * sh.ks * 64;
  const dim3 grid(rows_total / (16 * sh.R), sh.slices, sh.kz);
  size_t lds = pg_lds_bytes(wg / 64, sh.NT);
  if (sh.solo && lds < KH_PG_SOLO_LDS) lds = KH_PG_SOLO_LDS;  // one workgroup per CU at a time
  auto opt_in = [&](auto kern, dim3&) { return pg_lds_opt_in((const void*)kern, lds); };
  const int tile = pg_tile(sh.R, sh.NT);  // one that is not listed runs as (2,2) where R is 2, else as (1,4)
  bool launched = false;
  if (w16) {
    for (int j = 0; j < 3; ++j)
      if (on16.w[j]) a.w[j].w = on16.w[j];
    const int t = tile >= 0 ? tile : (sh.R == 2 ? 2 : 3);
    launched = pg_gemm_w16_launch(PgW16Launch{EPI, kPgTiles[t][0], kPgTiles[t][1], grid, wg, lds}, m->stream, a, p.tiles,
                                  p.lanes);
  } else if (q16) {
    // the int8 image's own weight and scale pointers, on the _q16 stem (kh_gemm_q16.h, compiled in kh_model_gemm_q16.hip)
    const int t = tile >= 1 ? tile : (sh.R == 2 ? 2 : 3);
    launched = pg_gemm_q16_launch(PgW16Launch{EPI, kPgTiles[t][0], kPgTiles[t][1], grid, wg, lds}, m->stream, a, p.tiles,
                                  p.lanes);
  } else {
    kh_pick_bool(m->cfg.is_quant, [&](auto Q) {
      kh_pick(KhVals<0, 1, 2, 3>{}, tile >= 0 ? tile : (sh.R == 2 ? 2 : 3), [&](auto I) {
        constexpr int R = kPgTiles[I][0], NT = kPgTiles[I][1];
        if (p.lanes) {
          if constexpr (NT <= 4)  // clamped above
            launched = kh_launch_prep(opt_in, KH_KERNEL(k_sg_gemm, Q, R, NT, EPI), grid, wg, lds, m->stream, a, *p.lanes);
          return;
        }
        if constexpr (EPI == KH_PG_QKV) {  // the other GEMMs do not care where a token sits
          if (p.tiles) {
            launched = kh_launch_prep(opt_in, KH_KERNEL(k_rg_gemm, Q, R, NT, EPI), grid, wg, lds, m->stream, a, *p.tiles);
            return;
          }
        }
        if constexpr (EPI != KH_PG_STORE)  // the classifier epilogue is the lanes' alone
          launched = kh_launch_prep(opt_in, KH_KERNEL(k_pg_gemm, Q, R, NT, EPI), grid, wg, lds, m->stream, a);
      });
    });
  }
  if (!launched) *ok = false;
  if (EPI == KH_PG_RESID) return sh.kz > 1 ? sh.kz : 0;
  return EPI == KH_PG_QKV && a.rope != KH_PG_ROPE_OFF;
}
// k_rg_attn (kh_seq_prefill.h) in k_pg_attn's launch geometry at one query tile per workgroup, with k_pg_attn's waves
// per head size; pg_attn_supported(head_size) is the caller's to check
void launch_rg_attn(const KhPgAttnArgs& a, const KhRgTiles& tiles, int head_size, hipStream_t s) {
  const int grid = a.kv_heads * a.kv_mul * (a.T / 16);
  switch (head_size) {
    case 48: kh_launch(KH_KERNEL(k_rg_attn, 3, 8), grid, 64 * 8, 0, s, a, tiles); break;
    case 64: kh_launch(KH_KERNEL(k_rg_attn, 4, 8), grid, 64 * 8, 0, s, a, tiles); break;
    case 128: kh_launch(KH_KERNEL(k_rg_attn, 8, 4), grid, 64 * 4, 0, s, a, tiles); break;
    default: break;
  }
}
// The layer driver (the table above PgPass).  false: the LDS opt-in of a GEMM shape was refused - that launch was
// skipped, the rest of the pass is enqueued, and the entry point answers KH_ERR_UNSUPPORTED.
bool launch_pg_pass(kh_model* m, const PgPass& p) {
  const kh_config& c = m->cfg;
  const bool q = c.is_quant;
  const int T = p.T, tcap = pg_tcap(T);  // tcap: token stride of this pass's tiled slabs
  bool ok = true;
  if (p.lanes) {
    launch_log("k_sg_embed");
    hipLaunchKernelGGL(k_sg_embed, dim3(T), dim3(KH_WG), 0, m->stream, (const int32_t*)m->d_seq_tok, *p.lanes,
                       c.vocab_size, (const float*)m->tok_emb, (float*)m->pg_x, c.dim);
  } else {
    (void)kh_embedding_f32_host(p.toks, T, m->tok_emb, m->pg_x, c.dim, c.vocab_size, (void*)m->stream);
  }
  int pending_kz = 0;  // K slices of the last residual GEMM still to be added to pg_x (by the next RMSNorm)
  auto rmsnorm = [&](const float* w) {
    kh_pick_bool(q, [&](auto Q) {
      kh_launch(KH_KERNEL(k_pg_rmsnorm, Q), T, KH_WG, 0, m->stream, (float*)m->pg_x, w, (float*)m->pg_xn, c.dim,
                c.rms_eps, tcap, (const float*)m->pg_part, pending_kz);
    });
    pending_kz = 0;
  };
  // what every GEMM of the pass reads or writes alike: B operand (tiled?), output rows and their stride, contraction
  auto gemm_args = [&](const float* B, int b_tiled, float* out, int rows0, int ldo, int K) {
    KhPgGemmArgs a{};
    a.B = B; a.b_tiled = b_tiled; a.tcap = tcap; a.out = out;
    a.rows0 = rows0; a.ldo = ldo; a.K = K; a.T = T; a.gshift = m->gshift;
    return a;
  };
  // attention of a run's or a tile table's slice: MFMA kernel (kh_pattn.h) unless KH_PG_ATTN=0 or an odd head size
  const bool mfma_attn = !p.lanes && pg_mfma_attn(m);
  const bool rope_fuse_env = !dbg_off("KH_PG_ROPE_FUSE");
  for (int l = 0; l < c.layer_num; ++l) {
    const LayerW& W = m->layers[l];
    const kh_model::WCopy::Layer C = m->w16.arena ? m->w16.layers[(size_t)l] : kh_model::WCopy::Layer{};  // (KH_FLAG_GEMM16)
    float* kc = m->kcache + (size_t)l * c.cache_len * c.kv_dim;
    float* vc = m->vcache + (size_t)l * c.cache_len * c.kv_dim;
    rmsnorm(W.att_norm);
    bool rope_fused = false;
    {
      KhPgGemmArgs a = gemm_args(m->pg_xn, 1, m->pg_q, c.dim, c.dim, c.dim);
      a.w[0] = W.wq; a.w[1] = W.wk; a.w[2] = W.wv;
      a.kc = kc; a.vc = vc; a.rows1 = c.kv_dim; a.pos0 = p.pos0;
      // RoPE in the epilogue: interleaved pairs sit in one lane's float4; half-mode partners need the
      // paired-tile mapping (R = 2, head size a multiple of 32).  KH_PG_ROPE_FUSE=0: separate kernel.
      a.head_size = c.head_size; a.sin_cache = m->sin_cache; a.cos_cache = m->cos_cache;
      a.rope = !rope_fuse_env ? KH_PG_ROPE_OFF
               : (c.rope_mode == KH_ROPE_HALF ? (c.head_size % 32 == 0 ? KH_PG_ROPE_TILES : KH_PG_ROPE_OFF)
                                              : KH_PG_ROPE_PAIRS);
      rope_fused = pg_gemm<KH_PG_QKV>(m, p, c.dim + 2 * c.kv_dim, c.dim % 32 == 0 && c.kv_dim % 32 == 0, a, &ok,
                                          PgOn16{KH_W16_QKV, {C.wq, C.wk, C.wv}}) != 0;
    }
    if (!rope_fused && p.lanes) {
      launch_log("k_sg_rope");
      hipLaunchKernelGGL(k_sg_rope, dim3(T), dim3(KH_WG), 0, m->stream, (float*)m->pg_q, kc,
                         (const float*)m->sin_cache, (const float*)m->cos_cache, c.dim, c.kv_dim, c.head_size, *p.lanes,
                         (int)c.rope_mode);
    } else if (!rope_fused && p.tiles) {
      launch_log("k_rg_rope");
      hipLaunchKernelGGL(k_rg_rope, dim3(T), dim3(KH_WG), 0, m->stream, m->pg_q, kc, m->sin_cache,
                         m->cos_cache, c.dim, c.kv_dim, c.head_size, *p.tiles, c.rope_mode);
    } else if (!rope_fused) {
      launch_log("k_pg_rope");
      hipLaunchKernelGGL(k_pg_rope, dim3(T), dim3(KH_WG), 0, m->stream, m->pg_q, kc, m->sin_cache,
                         m->cos_cache, c.dim, c.kv_dim, c.head_size, p.pos0, c.rope_mode);
    }
    // the prompt phase leaves K/V rows and nothing else (no logits): the last layer's K/V rows are
    // written, its attention, wo and FFN feed nothing (1/L of the pass minus one QKV GEMM) - unless the
    // classifier follows (full_depth)
    if (l == c.layer_num - 1 && !p.full_depth) break;
    if (p.lanes) {
      for (int g = 0; g < pg_lane_groups(p); ++g) {
        int ng;
        const KhSeqLanes lg = pg_lane_group(m, p, g, &ng);
        const size_t at = (size_t)g * KH_PF_BMAX * c.dim;
        seq_attn_enqueue(m, l, m->pg_q + at, m->pg_att + at, lg, ng);
      }
    } else if (mfma_attn) {
      KhPgAttnArgs a{};
      a.q = m->pg_q; a.kc = kc; a.vc = vc; a.out = m->pg_att;
      a.dim = c.dim; a.kv_dim = c.kv_dim; a.kv_heads = c.kv_head_num; a.kv_mul = c.kv_mul;
      a.T = T; a.pos0 = p.pos0; a.layout = q ? KH_PA_TILED_Q8 : KH_PA_TILED_F32; a.tcap = tcap;
      if (p.tiles)
        launch_rg_attn(a, *p.tiles, c.head_size, m->stream);
      else
        launch_pg_attn(a, c.head_size, m->stream);
    } else {
      // head sizes without an MFMA instantiation (and KH_PG_ATTN=0): the decode kernel, one grid
      // slice per token, 256-thread workgroups (4096 latency-bound (head, token) workgroups: twice
      // as many fit a CU as with the decode width, 28.7 -> 19.6 us per layer)
      launch_attn_decode(attn_slice_args(m, l, m->pg_q, m->pg_att, m->pg_ws, m->pg_ws_tok_bytes), p.pos0, KH_WG, m->stream,
                         T, p.pos0 + T - 1);
    }
    {
      // the decode kernels leave row-major rows
      KhPgGemmArgs a = gemm_args(m->pg_att, mfma_attn ? 1 : 0, m->pg_x, c.dim, c.dim, c.dim);
      a.w[0] = W.wo; a.part = m->pg_part;
      pending_kz = pg_gemm<KH_PG_RESID>(m, p, c.dim, c.dim % 32 == 0, a, &ok, PgOn16{KH_W16_WO, {C.wo}});
    }
    rmsnorm(W.ffn_norm);
    {
      KhPgGemmArgs a = gemm_args(m->pg_xn, 1, m->pg_h, c.hidden_dim, c.hidden_dim, c.dim);
      a.w[0] = W.w1; a.w[1] = W.w3;
      pg_gemm<KH_PG_SWIGLU>(m, p, c.hidden_dim, c.hidden_dim % 32 == 0, a, &ok, PgOn16{KH_W16_FFN13, {C.w1, C.w3}});
    }
    {
      KhPgGemmArgs a = gemm_args(m->pg_h, 1, m->pg_x, c.dim, c.dim, c.hidden_dim);
      a.w[0] = W.w2; a.part = m->pg_part;
      pending_kz = pg_gemm<KH_PG_RESID>(m, p, c.dim, c.dim % 32 == 0, a, &ok, PgOn16{KH_W16_W2, {C.w2}});  // (the next RMSNorm adds them)
    }
  }
  if (p.full_depth) {
    rmsnorm(m->final_norm);  // adds the last w2 GEMM's pending partials too
    KhPgGemmArgs a = gemm_args(m->pg_xn, 1, m->sg_logits, c.vocab_size, m->pf_vstride, c.dim);
    a.w[0] = m->cls;
    pg_gemm<KH_PG_STORE>(m, p, c.vocab_size, c.vocab_size % 32 == 0, a, &ok, PgOn16{KH_W16_CLS, {m->w16.cls}});
  }
  return ok;
}
}  // namespace

// Host-only view of the prefill GEMM launch plan (pg_shape) for tools and the CPU test-suite: epi 0 = QKV
// (rows = dim + 2 kv_dim), 1 = residual GEMM (wo / w2: rows = dim), 2 = SwiGLU pair (rows = hidden_dim); K =
// contraction length; r2_ok = the 32-row register tile divides the row blocks.  out[7] = {R, NT, ks, token
// slices, solo, kz, workgroups}.  No device is touched; the KH_PG_SHAPE_* overrides are not applied.
extern "C" int kh_plan_prefill_shape(int32_t epi, int32_t T, int32_t rows, int32_t K, int32_t is_quant,
                                     int32_t r2_ok, int32_t* out7) {
  if (!out7 || epi < 0 || epi > 2 || T <= 0 || T > KH_PG_TMAX || rows <= 0 || K <= 0) return KH_ERR_INVALID_ARG;
  const bool q = is_quant != 0;
  if (rows % 16 || K % (q ? 64 : 16)) return KH_ERR_UNSUPPORTED;
  const PgShape sh = pg_shape(T, rows, r2_ok != 0, epi == KH_PG_SWIGLU ? 2 : 1, K / (q ? 64 : 16), q ? 4 : 16, q,
                              epi == KH_PG_RESID);
  out7[0] = sh.R; out7[1] = sh.NT; out7[2] = sh.ks; out7[3] = sh.slices; out7[4] = sh.solo ? 1 : 0; out7[5] = sh.kz;
  out7[6] = rows / (16 * sh.R) * sh.slices * sh.kz;
  return KH_OK;
}

// ---- the GEMM prefill: T (<= KH_PG_TMAX) prompt tokens per pass at positions pos0.., fills their K/V cache rows ------
extern "C" int kh_model_prefill_gemm(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0) {
  int rc = khm::prefill_gemm_run(m, h_tokens, n, pos0);
  if (rc == KH_OK) rc = khm::lp_none(m, pos0, n);
  return rc == KH_OK ? khm::hist_write(m, h_tokens, n, pos0) : rc;
}
int khm::prefill_gemm_run(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0) {
  if (!m || !h_tokens || n <= 0 || pos0 < 0) return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  if ((int64_t)pos0 + n > c.cache_len) return KH_ERR_RANGE;
  if (!tokens_in_vocab(m, h_tokens, n)) return KH_ERR_RANGE;
  if (!pg_supported(m)) return KH_ERR_UNSUPPORTED;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  int rc;
  if ((rc = kv_ensure(m, pos0 + n)) != KH_OK) return rc;
  if ((rc = prefill_gemm_prepare(m)) != KH_OK) return rc;
  // tuning / test hook: KH_PG_CHUNK=<tokens per weight pass> (16 .. KH_PG_TMAX), read per call
  int chunk = KH_PG_TMAX;
  if (const char* e = dbg("KH_PG_CHUNK")) {
    const int v = atoi(e);
    chunk = v < 16 ? 16 : (v > KH_PG_TMAX ? KH_PG_TMAX : v);
  }
  bool ok = true;
  for (int t0 = 0; t0 < n; t0 += chunk)
    ok &= launch_pg_pass(m, pg_run(h_tokens + t0, n - t0 < chunk ? n - t0 : chunk, pos0 + t0));
  if (!ok) return KH_ERR_UNSUPPORTED;  // a GEMM shape's LDS opt-in was refused
  return kh_launch_status();
}

// ---- the GEMM prefill into sequence slots (kh_seq_prefill.h; kh_model_seq.hip checks the call and drives this) -------
int khm::seq_prefill_gemm_check(const kh_model* m) {
  // no fallback to the VALU pass, none to the decode-attention slices (KH_PG_ATTN=0 refuses the call)
  return pg_supported(m) && pg_mfma_attn(m) ? KH_OK : KH_ERR_UNSUPPORTED;
}
int khm::seq_prefill_gemm_enqueue(kh_model* m, int n_seq, const int32_t* slots, const int32_t* toks,
                                  const int32_t* n_tokens, const int32_t* pos0) {
  int rc;
  if ((rc = ensure_pg_buffers(m)) != KH_OK) return rc;
  std::vector<size_t> seg_at((size_t)n_seq);  // where segment s starts in toks
  size_t at = 0;
  for (int s = 0; s < n_seq; ++s) {
    seg_at[s] = at;
    at += (size_t)n_tokens[s];
  }
  KhRgTiles tiles;
  int32_t slab_tok[KH_PG_TMAX];
  int ntiles = 0, cur_pass = 0;
  bool ok = true;
  auto flush = [&]() {
    if (ntiles == 0) return;
    for (int k = ntiles; k < KH_RG_TILES; ++k) {  // entries no slab token reads: the last tile's, as the lane tables pad
      tiles.pos0[k] = tiles.pos0[ntiles - 1];
      tiles.nvalid[k] = tiles.nvalid[ntiles - 1];
      tiles.base[k] = tiles.base[ntiles - 1];
      tiles.pfx_len[k] = tiles.pfx_len[ntiles - 1];
      tiles.pfx_row0[k] = tiles.pfx_row0[ntiles - 1];
    }
    ok &= launch_pg_pass(m, pg_tiles(slab_tok, 16 * ntiles, tiles));
    ntiles = 0;
  };
  kh_rg_plan(n_seq, n_tokens, [&](int pass, int s, int off, int n) {
    if (pass != cur_pass) {
      flush();
      cur_pass = pass;
    }
    const KhSeqSlot& t = m->seq_tab[slots[s]];
    for (int o = 0; o < n; o += 16) {
      const int k = ntiles++, nv = n - o < 16 ? n - o : 16;
      tiles.pos0[k] = pos0[s] + off + o;
      tiles.nvalid[k] = nv;
      tiles.base[k] = kh_seq_own_base(t);
      tiles.pfx_len[k] = t.pfx;
      tiles.pfx_row0[k] = t.pfx > 0 ? m->seq_tab[t.parent].row0 : 0;
      // the padding tokens of a segment's last tile repeat its last valid token
      for (int i = 0; i < 16; ++i) slab_tok[16 * k + i] = toks[seg_at[s] + (size_t)(off + o + (i < nv ? i : nv - 1))];
    }
  });
  flush();
  if (!ok) return KH_ERR_UNSUPPORTED;  // a GEMM shape's LDS opt-in was refused
  return kh_launch_status();
}

// ---- the wide sequence pass (kh_seq_gemm.h): up to KH_SEQ_SLOTS_MAX lanes of distinct slots at full depth -------------
bool khm::seq_gemm_supported(const kh_model* m) {
  // the 8-lane pass's attention and tail (full_depth_supported: their buffers are seq_prepare's), the GEMMs' K and row
  // granules, and a classifier of whole 16-row tiles
  return full_depth_supported(m) && pg_supported(m) && m->cfg.vocab_size % 16 == 0;
}
int khm::seq_gemm_prepare(kh_model* m) {
  int rc;
  if ((rc = ensure_pg_buffers(m)) != KH_OK) return rc;
  if (m->sg_logits) return KH_OK;
  KhDev<float> lg;
  const size_t n = (size_t)KH_SEQ_SLOTS_MAX * (size_t)m->pf_vstride;  // pf_vstride: seq_prepare ran
  if ((rc = lg.alloc(n)) != KH_OK) return rc;
  KH_CHECK_HIP(hipMemsetAsync(lg, 0, n * sizeof(float), m->stream));
  m->sg_logits = std::move(lg);
  return KH_OK;
}
int khm::seq_pass_enqueue_gemm(kh_model* m, const int32_t* slots, const int32_t* pos, int n, bool words,
                               const KhSeqTail* tail) {
  if (n <= 0 || n > KH_SEQ_SLOTS_MAX) return KH_ERR_RANGE;
  KhWideLanes wide;
  for (int b = 0; b < KH_SEQ_SLOTS_MAX; ++b) {  // padding lanes repeat the last valid lane
    const int i = b < n ? b : n - 1;
    wide.pos[b] = pos[i];
    wide.row[b] = kh_seq_own_base(m->seq_tab[slots[i]]) + pos[i];
    wide.slot[b] = slots[i];
  }
  const PgPass p = pg_lanes(wide, slots, n);
  const bool ok = launch_pg_pass(m, p);
  m->sg_lanes = n;
  // the 8-lane pass's tail, once per group of KH_PF_BMAX lanes
  for (int g = 0; g < pg_lane_groups(p); ++g) {
    int ng, rc;
    const KhSeqLanes lg = pg_lane_group(m, p, g, &ng);
    if ((rc = seq_tail_enqueue(m, m->sg_logits + (size_t)g * KH_PF_BMAX * m->pf_vstride, lg, ng, words, tail)) != KH_OK)
      return rc;
  }
  if (!ok) return KH_ERR_UNSUPPORTED;  // a GEMM shape's LDS opt-in was refused
  return kh_launch_status();
}

// Operator-level entry of the MFMA slice attention (kh_pattn.h): the multi-token form of MHAKernel.
extern "C" int kh_mha_prefill_f32(int32_t pos0, int32_t n_tokens, int32_t head_num, int32_t layer_index,
                                  int32_t seq_len, int32_t kv_dim, int32_t kv_mul, int32_t head_size,
                                  float* mha_out, const float* q, const float* key_cache,
                                  const float* value_cache, void* stream) {
  if (!mha_out || !q || !key_cache || !value_cache) return KH_ERR_INVALID_ARG;
  if (n_tokens <= 0 || pos0 < 0 || head_num <= 0 || layer_index < 0 || seq_len <= 0 || kv_mul <= 0 ||
      head_size <= 0 || kv_dim <= 0)
    return KH_ERR_INVALID_ARG;
  if (head_num % kv_mul || kv_dim != (head_num / kv_mul) * head_size) return KH_ERR_INVALID_ARG;
  if ((int64_t)pos0 + n_tokens > seq_len) return KH_ERR_RANGE;
  if (!pg_attn_supported(head_size)) return KH_ERR_UNSUPPORTED;
  if (((uintptr_t)mha_out | (uintptr_t)q | (uintptr_t)key_cache | (uintptr_t)value_cache) & 15)
    return KH_ERR_INVALID_ARG;  // 16-byte loads / stores
  KhPgAttnArgs a{};
  const size_t layer_off = (size_t)layer_index * seq_len * kv_dim;
  a.q = q; a.kc = key_cache + layer_off; a.vc = value_cache + layer_off; a.out = mha_out;
  a.dim = head_num * head_size; a.kv_dim = kv_dim; a.kv_heads = head_num / kv_mul; a.kv_mul = kv_mul;
  a.T = n_tokens; a.pos0 = pos0; a.layout = KH_PA_ROWS;
  launch_pg_attn(a, head_size, (hipStream_t)stream);
  return kh_launch_status();
}

namespace {
// What kh_mha_prefill_f32 checks of the head geometry, the caches and the pointers, for the two entries below; on
// KH_OK `a` holds everything but the query columns (T, pos0), the layout and tcap.
int pa_op_args(KhPgAttnArgs& a, int32_t head_num, int32_t layer_index, int32_t seq_len, int32_t kv_dim, int32_t kv_mul,
               int32_t head_size, float* mha_out, const float* q, const float* key_cache, const float* value_cache) {
  if (!mha_out || !q || !key_cache || !value_cache) return KH_ERR_INVALID_ARG;
  if (head_num <= 0 || layer_index < 0 || seq_len <= 0 || kv_mul <= 0 || head_size <= 0 || kv_dim <= 0)
    return KH_ERR_INVALID_ARG;
  if (head_num % kv_mul || kv_dim != (head_num / kv_mul) * head_size) return KH_ERR_INVALID_ARG;
  if (!pg_attn_supported(head_size)) return KH_ERR_UNSUPPORTED;
  if (((uintptr_t)mha_out | (uintptr_t)q | (uintptr_t)key_cache | (uintptr_t)value_cache) & 15)
    return KH_ERR_INVALID_ARG;  // 16-byte loads / stores
  const size_t layer_off = (size_t)layer_index * seq_len * kv_dim;
  a.q = q; a.kc = key_cache + layer_off; a.vc = value_cache + layer_off; a.out = mha_out;
  a.dim = head_num * head_size; a.kv_dim = kv_dim; a.kv_heads = head_num / kv_mul; a.kv_mul = kv_mul;
  return KH_OK;
}
bool pa_op_layout(int32_t layout, int32_t tcap, int32_t T, int dim) {
  if (layout != KH_PA_TILED_F32 && layout != KH_PA_TILED_Q8 && layout != KH_PA_ROWS) return false;
  // the int8 slab interleaves the quarters of 64-column blocks (pg_tiled_index): a partial block would reach past
  // dim * tcap floats (an int8 model's dim is a multiple of its group size)
  if (layout == KH_PA_TILED_Q8 && dim % 64) return false;
  return T <= tcap && tcap <= KH_PG_TMAX && tcap % 16 == 0;
}
}  // namespace

// kh_mha_prefill_f32 in the output layout a model pass asks for (kh_pattn.h: KH_PA_TILED_F32 / KH_PA_TILED_Q8 /
// KH_PA_ROWS); the tiled layouts write a slab of dim x tcap floats (pg_tiled_index).
extern "C" int kh_mha_prefill_layout_f32(int32_t pos0, int32_t n_tokens, int32_t head_num, int32_t layer_index,
                                         int32_t seq_len, int32_t kv_dim, int32_t kv_mul, int32_t head_size,
                                         int32_t layout, int32_t tcap, float* mha_out, const float* q,
                                         const float* key_cache, const float* value_cache, void* stream) {
  KhPgAttnArgs a{};
  if (n_tokens <= 0 || pos0 < 0) return KH_ERR_INVALID_ARG;
  const int rc = pa_op_args(a, head_num, layer_index, seq_len, kv_dim, kv_mul, head_size, mha_out, q, key_cache,
                            value_cache);
  if (rc != KH_OK) return rc;
  if (!pa_op_layout(layout, tcap, n_tokens, a.dim)) return KH_ERR_INVALID_ARG;
  if ((int64_t)pos0 + n_tokens > seq_len) return KH_ERR_RANGE;
  a.T = n_tokens; a.pos0 = pos0; a.layout = layout; a.tcap = tcap;
  launch_pg_attn(a, head_size, (hipStream_t)stream);
  return kh_launch_status();
}

// Operator-level entry of the slot prefill's attention (kh_seq_prefill.h: k_rg_attn): n_tiles query tiles of 16 slab
// tokens each, tile k described by h_tiles[0..5)[k] = pos0, nvalid, base, pfx_len, pfx_row0 (KhRgTiles).  Every cache
// row a tile may read must lie in [0, seq_len).
extern "C" int kh_mha_prefill_tiles_f32(int32_t n_tiles, const int32_t* h_tiles, int32_t head_num,
                                        int32_t layer_index, int32_t seq_len, int32_t kv_dim, int32_t kv_mul,
                                        int32_t head_size, int32_t layout, int32_t tcap, float* mha_out,
                                        const float* q, const float* key_cache, const float* value_cache,
                                        void* stream) {
  KhPgAttnArgs a{};
  if (!h_tiles || n_tiles < 1 || n_tiles > KH_RG_TILES) return KH_ERR_INVALID_ARG;
  const int rc = pa_op_args(a, head_num, layer_index, seq_len, kv_dim, kv_mul, head_size, mha_out, q, key_cache,
                            value_cache);
  if (rc != KH_OK) return rc;
  if (!pa_op_layout(layout, tcap, 16 * n_tiles, a.dim)) return KH_ERR_INVALID_ARG;
  KhRgTiles tiles;
  for (int k = 0; k < KH_RG_TILES; ++k) {  // entries no slab token reads: the last tile's
    const int s = k < n_tiles ? k : n_tiles - 1;
    const int64_t pos0 = h_tiles[s], nv = h_tiles[n_tiles + s], base = h_tiles[2 * n_tiles + s];
    const int64_t pfx = h_tiles[3 * n_tiles + s], prow = h_tiles[4 * n_tiles + s];
    if (nv < 1 || nv > 16 || pos0 < 0 || pfx < 0 || pfx > pos0) return KH_ERR_INVALID_ARG;
    if (pfx > 0 && (prow < 0 || prow + pfx > seq_len)) return KH_ERR_RANGE;  // rows pfx_row0 + [0, pfx_len)
    if (base + pfx < 0 || base + pos0 + nv > seq_len) return KH_ERR_RANGE;   // rows base + [pfx_len, pos0 + nvalid)
    tiles.pos0[k] = (int32_t)pos0; tiles.nvalid[k] = (int32_t)nv; tiles.base[k] = (int32_t)base;
    tiles.pfx_len[k] = (int32_t)pfx; tiles.pfx_row0[k] = (int32_t)prow;
  }
  a.T = 16 * n_tiles; a.pos0 = 0; a.layout = layout; a.tcap = tcap;
  launch_rg_attn(a, tiles, head_size, (hipStream_t)stream);
  return kh_launch_status();
}
