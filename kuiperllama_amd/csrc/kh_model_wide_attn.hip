// kh_model_wide_attn.hip — the wide sequence pass's attention in one launch per layer for all lanes, shared prefixes
// read once (KH_FLAG_WIDE_ATTN; kh_seq_attn_wide.h: k_sg_attn, k_sg_attn_merge; the plan is kh_wide_attn_plan.h).  This
// translation unit compiles the kernels, keeps the flag's state and the partial workspace of a model, builds a pass's
// item table from its lanes and the slot table, and holds the operator-level entry kh_mha_decode_lanes_f32 and the
// host-only kh_plan_wide_attn.  kh_model_gemm.hip's layer driver calls wide_attn_enqueue in place of its loop over
// groups of 8 lanes.  The reference attends one sequence per process (cuda/mha_kernel.cu:47-110).
// gfx950 only.
#include <string.h>

#include "kh_dispatch.h"
#include "kh_model_internal.h"
#include "kh_pattn.h"  // pg_attn_supported
#include "kh_seq_attn_wide.h"
#include "kh_seq_gemm.h"

namespace khm {
namespace {
// Both launches of one layer.  Head sizes: pg_attn_supported's, with k_pg_attn's waves and its largest query-tile
// count per head size (kh_wa_qt, which the table's units were counted with).
void wa_launch(const KhSgAttnArgs& a, const KhWaTable& t, int head_size, hipStream_t s) {
  const int grid = t.unit0[t.n_items] * a.kv_heads, rows = t.n_lanes * a.kv_heads * a.kv_mul;
  switch (head_size) {
    case 48:
      kh_launch(KH_KERNEL(k_sg_attn, 3, 8, 4), grid, 64 * 8, 0, s, a, t);
      kh_launch(KH_KERNEL(k_sg_attn_merge, 3), rows, 64, 0, s, a, t);
      break;
    case 64:
      kh_launch(KH_KERNEL(k_sg_attn, 4, 8, 4), grid, 64 * 8, 0, s, a, t);
      kh_launch(KH_KERNEL(k_sg_attn_merge, 4), rows, 64, 0, s, a, t);
      break;
    case 128:
      kh_launch(KH_KERNEL(k_sg_attn, 8, 4, 2), grid, 64 * 4, 0, s, a, t);
      kh_launch(KH_KERNEL(k_sg_attn_merge, 8), rows, 64, 0, s, a, t);
      break;
    default: break;
  }
}
}  // namespace

// Read at creation.  Hook KH_WIDE_ATTN=1 / 0 overrides the flag.
void wide_attn_configure(kh_model* m) {
  kh_model::WideAttn& w = m->wattn;
  w.on = false;
  const char* hook = dbg("KH_WIDE_ATTN");
  const bool want = hook ? hook[0] == '1' : (m->opts.flags & KH_FLAG_WIDE_ATTN) != 0;
  if (!want) { w.reason = KH_WIDE_ATTN_NO_FLAG; return; }
  if (!seq_gemm_supported(m)) { w.reason = KH_WIDE_ATTN_GEOMETRY; return; }
  if (!pg_attn_supported(m->cfg.head_size)) { w.reason = KH_WIDE_ATTN_HEAD_SIZE; return; }
  w.on = true;
  w.reason = KH_WIDE_ATTN_ON;
}

int wide_attn_prepare(kh_model* m) {
  if (!m->wattn.on || m->wattn.ws) return KH_OK;
  KhDev<float> ws;
  int rc;
  // every slot a merge reads was written by the k_sg_attn launch before it: no clearing
  if ((rc = ws.alloc(kh_wa_ws_floats(KH_SEQ_SLOTS_MAX, m->cfg.head_num, m->cfg.head_size))) != KH_OK) return rc;
  m->wattn.ws = std::move(ws);
  return KH_OK;
}

void wide_attn_table(const kh_model* m, const KhWideLanes& lanes, const int32_t* slots, int n, KhWaTable* t) {
  int32_t tab[4 * KH_SEQ_SLOTS_MAX];
  for (int i = 0; i < n; ++i) {
    const KhSeqSlot& s = m->seq_tab[slots[i]];
    tab[i] = lanes.pos[i];
    tab[n + i] = lanes.row[i] - lanes.pos[i];
    tab[2 * n + i] = s.pfx;
    tab[3 * n + i] = s.pfx > 0 ? m->seq_tab[s.parent].row0 : 0;
  }
  kh_wa_plan(n, tab, m->cfg.kv_mul, kh_wa_qt(m->cfg.head_size), t);
}

void wide_attn_enqueue(kh_model* m, int l, const float* q, float* out, const KhWaTable& t) {
  const kh_config& c = m->cfg;
  KhSgAttnArgs a{};
  a.q = q; a.out = out; a.ws = m->wattn.ws;
  a.kc = m->kcache + (size_t)l * c.cache_len * c.kv_dim;
  a.vc = m->vcache + (size_t)l * c.cache_len * c.kv_dim;
  a.dim = c.dim; a.kv_dim = c.kv_dim; a.kv_heads = c.kv_head_num; a.kv_mul = c.kv_mul;
  wa_launch(a, t, c.head_size, m->stream);
}
}  // namespace khm
using namespace khm;

// out[8] = on (0 / 1), the reason where inert (KH_WIDE_ATTN_*), bytes of the partial workspace (0 before the first wide
// call under the flag), KH_WA_NSPLIT_MAX, query columns per K/V row read (16 x the tiles of a workgroup); 5 - 7 are 0.
extern "C" int kh_model_wide_attn_info(kh_model* m, int64_t* out) {
  if (!m || !out) return KH_ERR_INVALID_ARG;
  memset(out, 0, 8 * sizeof(int64_t));
  out[0] = m->wattn.on;
  out[1] = m->wattn.reason;
  out[2] = m->wattn.ws ? (int64_t)(kh_wa_ws_floats(KH_SEQ_SLOTS_MAX, m->cfg.head_num, m->cfg.head_size) * sizeof(float)) : 0;
  out[3] = KH_WA_NSPLIT_MAX;
  out[4] = 16 * kh_wa_qt(m->cfg.head_size);
  return KH_OK;
}

// Host-only view of the item table (kh_wide_attn_plan.h) for tools and the CPU suite.  h_lanes: int32 [4][n] - pos, base
// (= row - pos), pfx_len, pfx_row0; seq_len <= 0: row ranges are not checked against a cache.  out_items[8 * i ..] =
// {kind (0 share, 1 own), row0, len, chunks, 16-position tiles per chunk, lanes, first index in out_lanes, work units per
// kv head}, share items first, then lane i's own item at n_share + i; out_lanes: the items' lanes, item after item.
// *n_items = the items there are (KH_ERR_RANGE when cap_items holds fewer; out_items / out_lanes may then be NULL).
extern "C" int kh_plan_wide_attn(int32_t n_lanes, const int32_t* h_lanes, int32_t kv_mul, int32_t head_size,
                                 int32_t seq_len, int32_t* out_items, int32_t cap_items, int32_t* n_items,
                                 int32_t* out_lanes) {
  if (!n_items || kv_mul <= 0 || head_size <= 0) return KH_ERR_INVALID_ARG;
  const int rc = kh_wa_check(n_lanes, h_lanes, seq_len > 0 ? seq_len : INT32_MAX);
  if (rc != 0) return rc;
  KhWaTable t;
  kh_wa_plan(n_lanes, h_lanes, kv_mul, kh_wa_qt(head_size), &t);
  *n_items = t.n_items;
  if (cap_items < t.n_items || !out_items || !out_lanes) return KH_ERR_RANGE;
  for (int k = 0; k < t.n_items; ++k) {
    int32_t* o = out_items + 8 * k;
    o[0] = k < t.n_share ? 0 : 1; o[1] = t.row0[k]; o[2] = t.len[k]; o[3] = t.nsplit[k]; o[4] = t.ctiles[k];
    o[5] = t.nlanes[k]; o[6] = t.lane0[k]; o[7] = t.unit0[k + 1] - t.unit0[k];
    for (int i = 0; i < t.nlanes[k]; ++i) out_lanes[t.lane0[k] + i] = t.order[t.lane0[k] + i];
  }
  return KH_OK;
}

// Operator-level entry of the wide pass's attention: n_lanes query rows q[n][dim] of different sequences, lane i at
// position pos[i] with its positions [pfx_len, pos] at cache rows base + position and [0, pfx_len) at rows pfx_row0 +
// position (h_lanes: host int32 [4][n] - pos, base, pfx_len, pfx_row0), against rows of layer layer_index of caches
// [layers][seq_len][kv_dim]; mha_out[n][dim] row-major.  Runs the plan, k_sg_attn and k_sg_attn_merge with a workspace it
// allocates, synchronises the stream and frees.  Before any launch: KH_ERR_INVALID_ARG for NULL or misaligned pointers,
// a bad head geometry, n outside 1 .. 64, pos < pfx_len or a negative prefix; KH_ERR_RANGE for a row range outside
// [0, seq_len); KH_ERR_UNSUPPORTED for a head size other than 48 / 64 / 128.
extern "C" int kh_mha_decode_lanes_f32(int32_t n_lanes, const int32_t* h_lanes, int32_t head_num, int32_t layer_index,
                                       int32_t seq_len, int32_t kv_dim, int32_t kv_mul, int32_t head_size,
                                       float* mha_out, const float* q, const float* key_cache,
                                       const float* value_cache, void* stream) {
  if (!mha_out || !q || !key_cache || !value_cache || !h_lanes) return KH_ERR_INVALID_ARG;
  if (head_num <= 0 || layer_index < 0 || seq_len <= 0 || kv_mul <= 0 || head_size <= 0 || kv_dim <= 0)
    return KH_ERR_INVALID_ARG;
  if (head_num % kv_mul || kv_dim != (head_num / kv_mul) * head_size) return KH_ERR_INVALID_ARG;
  if (!pg_attn_supported(head_size)) return KH_ERR_UNSUPPORTED;
  if (((uintptr_t)mha_out | (uintptr_t)q | (uintptr_t)key_cache | (uintptr_t)value_cache) & 15)
    return KH_ERR_INVALID_ARG;  // 16-byte loads / stores
  const int rc = kh_wa_check(n_lanes, h_lanes, seq_len);
  if (rc != 0) return rc;
  KhWaTable t;
  kh_wa_plan(n_lanes, h_lanes, kv_mul, kh_wa_qt(head_size), &t);
  KhDev<float> ws;
  int arc;
  if ((arc = ws.alloc(kh_wa_ws_floats(n_lanes, head_num, head_size))) != KH_OK) return arc;
  KhSgAttnArgs a{};
  const size_t layer_off = (size_t)layer_index * seq_len * kv_dim;
  a.q = q; a.kc = key_cache + layer_off; a.vc = value_cache + layer_off; a.ws = ws; a.out = mha_out;
  a.dim = head_num * head_size; a.kv_dim = kv_dim; a.kv_heads = head_num / kv_mul; a.kv_mul = kv_mul;
  wa_launch(a, t, head_size, (hipStream_t)stream);
  const int lrc = kh_launch_status();
  KH_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));  // the workspace is freed on return
  return lrc;
}
