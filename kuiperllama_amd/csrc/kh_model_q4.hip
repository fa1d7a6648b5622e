// kh_model_q4.hip — Q4 at the model level: the packed 4-bit copy of a 4-bit-exact int8 model's matrices (plan, range
// check, release, the class masks of decode and of the B-token passes) and kh_model_q4_info.  The bytes, the build and
// the launch routing of a copy are kh_model_w16.hip's, shared with W16; the launch text is kh_copy_launch.h's,
// instantiated here for KH_SRC_Q4, which compiles the kh_q4.h kernels here and nowhere else (the pass kernels of
// kh_q4_pass.h: kh_model_q4_pass.hip).  Each launch is the int8 launch of kh_model_step.hip with the
// same shape (split, u, grid, wg - a shape forced through KH_SHAPE_* included) on the Q4 twin of its kernel, so the
// bits do not change.
// Replaces nothing in the reference (it streams int8 weights: kuiper/source/op/kernels/cuda/matmul_kernel.cu:56-87).
// gfx950 only.  No CPU fallback: every path below launches HIP kernels.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kh_q4.h"
#include "kh_copy_launch.h"

namespace khm {

KH_COPY_LAUNCHES(, KH_SRC_Q4);

namespace {
// Launch classes that run on the copy unless KH_Q4_CLASSES says otherwise: those that pass 3.1c's adoption rule - the Q4
// median below the flag-off median by more than the range of the flag-off runs - on both geometries of the same-box
// A/B (tools/q4_ab.py, profiles/q4_ab.txt).  qkv and wo are out: both pass at Llama-2-7B geometry (10.91
// -> 9.45 us, 5.09 -> 4.61 us) and lose at TinyLlama's (3.36 -> 3.54 us, 2.82 -> 2.84 us); KH_Q4_CLASSES=0x1f puts them
// back.  A class that is out keeps its int8 launch and costs nothing but its bytes in the copy.
enum { KH_Q4_DEFAULT = KH_W16_FFN13 | KH_W16_W2 | KH_W16_CLS };
size_t q4_mat_bytes(size_t elems) { return elems / 2; }
}  // namespace

int plan_q4(bool quant, int dim, int hidden_dim, int kv_dim, int vocab_size, int layer_num, int group_size,
            size_t* bytes) {
  if (bytes) *bytes = 0;
  if (!quant || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0 || layer_num <= 0) return 0;
  // a lane's unit is sixteen columns of one group (the int8 view's own premise)
  if (group_size < 16 || (group_size & (group_size - 1)) != 0 || dim % group_size != 0 || hidden_dim % group_size != 0)
    return 0;
  if (bytes) *bytes = copy_bytes(dim, hidden_dim, kv_dim, vocab_size, layer_num, q4_mat_bytes);
  return KH_Q4_DEFAULT;
}

void q4_release(kh_model* m) {
  kh_model::Q4& q = m->q4;
  if (q.classes & KH_W16_CLS) m->nparts = q.nparts_image;  // the int8 classifier launch's partials again
  copy_release(q);
  q.pass_classes = 0;
}

// Hook KH_Q4_CLASSES, read at creation: unset - the plan's classes; a number (strtol, base 0: 0x1f, 12, 0x1 for qkv
// alone, 0 for none) - a mask of KH_W16_* bits, whatever the plan says (the tests reach every kernel through it)
static int q4_class_mask(int planned) {
  const char* hook = dbg("KH_Q4_CLASSES");
  return hook ? (int)strtol(hook, nullptr, 0) & KH_W16_ALL : planned;
}

// Which classes run their B-token pass (kh_q4_pass.h) on the copy.  Hook KH_Q4_PASS, read at creation: unset or 1 -
// KH_Q4_PASS_DEFAULT; 0 - none (the passes stream int8 while decode reads the copy); any other number (strtol, base 0:
// 0x1f all, 0x1 qkv alone) - a mask of KH_W16_* bits.  Whatever KH_Q4_CLASSES says: the copy holds every matrix, and a
// 4-token pass has another balance than the short decode launches that kept qkv and wo on int8.
static int q4_pass_mask() {
  const char* hook = dbg("KH_Q4_PASS");
  if (!hook || strcmp(hook, "1") == 0) return KH_Q4_PASS_DEFAULT;
  return (int)strtol(hook, nullptr, 0) & KH_W16_ALL;
}

// All or nothing: one value outside [-8, 7] anywhere and the model launches what it launches without the flag.
int q4_create(kh_model* m) {
  const kh_config& c = m->cfg;
  kh_model::Q4& q = m->q4;
  q = kh_model::Q4();
  const char* hook = dbg("KH_Q4");
  const bool want = hook ? hook[0] == '1' : (m->opts.flags & KH_FLAG_Q4) != 0;
  if (!want) return KH_OK;
  size_t bytes = 0;
  const int planned =
      plan_q4(c.is_quant != 0, c.dim, c.hidden_dim, c.kv_dim, c.vocab_size, c.layer_num, c.group_size, &bytes);
  if (!bytes) return KH_OK;  // fp32, or a geometry the view does not cover: nothing changes
  int rc = copy_build(m, q, k_q4_build, q4_mat_bytes, 16, bytes, &q.first_inexact);
  if (rc != KH_OK) {
    q4_release(m);
    return rc;
  }
  if (q.first_inexact >= 0) {  // the model streams int8 as if no flag were set
    q4_release(m);
    q.state = -1;
    return KH_OK;
  }
  const int classes = q4_class_mask(planned);
  // A classifier on the copy launches the register-tile grid where the model planned the ring kernel's: the argmax
  // partials follow it (room for the larger of the two, so that a copy given up later needs no allocation)
  q.nparts_image = m->nparts;
  if ((classes & KH_W16_CLS) && m->sh_cls.grid != m->nparts) {
    if (m->sh_cls.grid > m->nparts) {
      KhDev<float> pv;
      KhDev<int32_t> pi;
      if ((rc = pv.alloc((size_t)m->sh_cls.grid)) != KH_OK || (rc = pi.alloc((size_t)m->sh_cls.grid)) != KH_OK) {
        q4_release(m);
        return rc;
      }
      m->part_val = std::move(pv);
      m->part_idx = std::move(pi);
    }
    m->nparts = m->sh_cls.grid;
  }
  q.bytes = bytes;
  copy_configure<KH_SRC_Q4>(m);
  q.classes = classes;
  q.pass_classes = q4_pass_mask();  // no launch here: the pass kernels' LDS opt-in is pf_clip_grid's, at their first launch
  q.state = 1;
  if (dbg("KH_LOAD_DEBUG") || dbg("KH_SHAPE_DEBUG"))
    fprintf(stderr, "[kh] Q4: %.1f MiB 4-bit copy of %d matrices in %.0f us, classes 0x%x, pass classes 0x%x\n",
            (double)bytes / (1 << 20), 7 * c.layer_num + 1, (double)q.build_us, (unsigned)classes, (unsigned)q.pass_classes);
  return KH_OK;
}

}  // namespace khm
using namespace khm;

// out2 = {KH_W16_* bits of the launch classes that run on the 4-bit copy (0: not applicable), bytes of the copy}
extern "C" int kh_plan_q4(int32_t dim, int32_t hidden_dim, int32_t kv_dim, int32_t vocab_size, int32_t layer_num,
                          int32_t is_quant, int32_t group_size, int64_t* out2) {
  if (!out2 || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0 || layer_num <= 0) return KH_ERR_INVALID_ARG;
  size_t bytes = 0;
  out2[0] = plan_q4(is_quant != 0, dim, hidden_dim, kv_dim, vocab_size, layer_num, group_size, &bytes);
  out2[1] = (int64_t)bytes;
  return KH_OK;
}

// out[0..5] = state, bytes, build us, class mask, first inexact tensor, class mask of the B-token passes
extern "C" int kh_model_q4_info(kh_model* m, int64_t* out) {
  if (!m || !out) return KH_ERR_INVALID_ARG;
  memset(out, 0, 8 * sizeof(int64_t));
  out[0] = m->q4.state;
  out[1] = (int64_t)m->q4.bytes;
  out[2] = (int64_t)m->q4.build_us;
  out[3] = m->q4.classes;
  out[4] = m->q4.first_inexact;
  out[5] = m->q4.pass_classes;
  return KH_OK;
}
