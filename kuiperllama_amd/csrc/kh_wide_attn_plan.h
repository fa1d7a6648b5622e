// kh_wide_attn_plan.h — host-only plan of the wide pass's one-launch attention (kh_seq_attn_wide.h, KH_FLAG_WIDE_ATTN):
// from the lanes of a pass to the ITEM table the kernel walks.  An item is one contiguous range of cache rows plus the
// pass lanes that attend to ALL of it:
//   share item  one per distinct (pfx_row0, pfx_len > 0) among the lanes: rows pfx_row0 + [0, pfx_len), its lanes are all
//               lanes with that pair (two sharers of one parent with different P are two items; the parent's own lane is
//               an ordinary own item)
//   own item    one per lane: positions [pfx_len, pos] at rows base + position, base = row - pos (negative for a sharer
//               near the start of the cache); at least one row
// Share items come first (they are the long ones and are dispatched first), own item of lane i is item n_share + i.
// An item's query COLUMNS are (lane in item, head j of the kv group), lanes x kv_mul of them, in tiles of 16; a
// workgroup takes `qt` tiles.  Its rows are cut into nsplit chunks of whole 16-position tiles.  The reference attends
// one sequence at a time (cuda/mha_kernel.cu:47-110).  No device code: kh_plan_wide_attn shows the table to the CPU suite.
#pragma once
#include <stdint.h>

#include "kh_seq_plan.h"  // KH_SEQ_SLOTS_MAX

#define KH_WA_ITEMS_MAX (2 * KH_SEQ_SLOTS_MAX)
#define KH_WA_NSPLIT_MAX 8        // chunks of an item: the partial workspace holds 2 x this many rows per (lane, head)
#define KH_WA_CHUNK_MIN_TILES 16  // a chunk is at least 256 positions: two tiles for each of a workgroup's 8 waves

// By value beside KhSgAttnArgs (kh_seq_attn_wide.h asserts the 4 KiB of kernel arguments).
struct KhWaTable {
  int32_t row0[KH_WA_ITEMS_MAX], len[KH_WA_ITEMS_MAX];  // rows row0 + [0, len)
  int32_t unit0[KH_WA_ITEMS_MAX + 1];  // item i owns the work units [unit0[i], unit0[i + 1]) of every kv head:
                                       // unit = chunk * groups + group of qt column tiles
  int32_t ctiles[KH_WA_ITEMS_MAX];     // 16-position tiles per chunk
  uint8_t nsplit[KH_WA_ITEMS_MAX];     // chunks
  uint8_t lane0[KH_WA_ITEMS_MAX], nlanes[KH_WA_ITEMS_MAX];  // the item's lanes are order[lane0 .. lane0 + nlanes)
  uint8_t order[KH_WA_ITEMS_MAX];      // the sharing lanes grouped by share item, then lanes 0 .. n_lanes - 1 (own items)
  uint8_t share_of[KH_SEQ_SLOTS_MAX];  // the lane's share item, 255: none
  int32_t n_items, n_share, n_lanes, qt;
};

// chunks of a range of len rows: one below 2 x KH_WA_CHUNK_MIN_TILES tiles, then as many as keep every chunk at
// KH_WA_CHUNK_MIN_TILES tiles or more, KH_WA_NSPLIT_MAX at the most; every chunk holds a row
static inline void kh_wa_chunks(int len, int* nsplit, int* ctiles) {
  const int tiles = (len + 15) / 16;
  int ns = tiles / KH_WA_CHUNK_MIN_TILES;
  ns = ns < 1 ? 1 : (ns > KH_WA_NSPLIT_MAX ? KH_WA_NSPLIT_MAX : ns);
  *ctiles = (tiles + ns - 1) / ns;
  *nsplit = (tiles + *ctiles - 1) / *ctiles;
}
// query tiles per workgroup (registers: head size 128 holds two, as k_pg_attn)
static inline int kh_wa_qt(int head_size) { return head_size == 128 ? 2 : 4; }

// What a lane table must satisfy before anything is planned or launched: 0, or -1 (an argument: n outside 1 .. 64,
// pos < pfx_len, a negative prefix) / -6 (a row range outside [0, seq_len)) - KH_ERR_INVALID_ARG / KH_ERR_RANGE.
// lanes: int32 [4][n] - pos, base (= row - pos), pfx_len, pfx_row0.
static inline int kh_wa_check(int n, const int32_t* lanes, int seq_len) {
  if (!lanes || n < 1 || n > KH_SEQ_SLOTS_MAX) return -1;
  for (int i = 0; i < n; ++i) {
    const int64_t pos = lanes[i], base = lanes[n + i], pfx = lanes[2 * n + i], prow = lanes[3 * n + i];
    if (pfx < 0 || pos < pfx) return -1;
    if (base + pfx < 0 || base + pos >= seq_len) return -6;       // rows base + [pfx_len, pos]
    if (pfx > 0 && (prow < 0 || prow + pfx > seq_len)) return -6;  // rows pfx_row0 + [0, pfx_len)
  }
  return 0;
}

// The table of a checked lane table (kh_wa_check) for kv_mul heads per kv group and qt column tiles per workgroup.
static inline void kh_wa_plan(int n, const int32_t* lanes, int kv_mul, int qt, KhWaTable* t) {
  const int32_t *pos = lanes, *base = lanes + n, *pfx = lanes + 2 * n, *prow = lanes + 3 * n;
  *t = KhWaTable();
  t->n_lanes = n;
  t->qt = qt;
  int ns = 0, at = 0;
  for (int i = 0; i < n; ++i) {  // share items in the order their first lane appears
    t->share_of[i] = 255;
    if (pfx[i] <= 0) continue;
    int s = 0;
    while (s < ns && !(t->row0[s] == prow[i] && t->len[s] == pfx[i])) ++s;
    if (s == ns) {
      t->row0[s] = prow[i];
      t->len[s] = pfx[i];
      ++ns;
    }
    t->share_of[i] = (uint8_t)s;
    ++t->nlanes[s];
  }
  for (int s = 0; s < ns; ++s) {
    t->lane0[s] = (uint8_t)at;
    for (int i = 0; i < n; ++i)
      if (t->share_of[i] == s) t->order[at++] = (uint8_t)i;
  }
  for (int i = 0; i < n; ++i) {  // own items: order[at + i] = i
    const int k = ns + i;
    t->row0[k] = base[i] + pfx[i];
    t->len[k] = pos[i] - pfx[i] + 1;
    t->lane0[k] = (uint8_t)(at + i);
    t->nlanes[k] = 1;
    t->order[at + i] = (uint8_t)i;
  }
  t->n_share = ns;
  t->n_items = ns + n;
  for (int k = 0; k < t->n_items; ++k) {
    int nsplit, ctiles;
    kh_wa_chunks(t->len[k], &nsplit, &ctiles);
    t->nsplit[k] = (uint8_t)nsplit;
    t->ctiles[k] = ctiles;
    const int col_tiles = (t->nlanes[k] * kv_mul + 15) / 16;
    t->unit0[k + 1] = t->unit0[k] + nsplit * ((col_tiles + qt - 1) / qt);
  }
  for (int k = t->n_items; k < KH_WA_ITEMS_MAX; ++k) t->unit0[k + 1] = t->unit0[t->n_items];
}
