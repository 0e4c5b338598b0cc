// packed.cpp — the packed verdict form's host entries (include/kwgpu.h): the dictionary of a pass
// from the environment, the decode functions and the host-encoder diagnostic. The arithmetic is
// packed.hpp's; the device pass is bulk.cpp's, its packed form bulkout.cpp's.
#include "packed.hpp"

#include "upload.hpp"

namespace kw {

int packed_dict(const Env& E, const int32_t* policies, uint32_t npol, int origin, uint32_t* dict) {
  if (!policies || !dict || (origin != KW_ORIGIN_VALIDATE && origin != KW_ORIGIN_AUDIT)) return KW_E_ARG;
  for (uint32_t j = 0; j < npol; ++j) {
    if (policies[j] < 0 || (size_t)policies[j] >= E.nvisible) return KW_E_ARG;
    const PolicyRec& P = E.pol[(size_t)policies[j]];
    uint32_t* d = dict + 3 * (size_t)j;
    if (P.init_error)
      packed_dict_const(kInitErrorWord, d);
    else if (P.is_group && (!P.prog.valid || P.prog.eval_error))
      packed_dict_const(finish_word(P.mode, 0, origin, KW_R_GROUP_EXPR, 0, false), d);
    else
      packed_dict_entry(P.mode, P.is_group ? 0u : (uint32_t)P.allowed_to_mutate, origin, d);
  }
  return KW_OK;
}

}  // namespace kw

extern "C" {

int kw_validate_host_packed(const kw_env* env, kw_batch* b, const int32_t* policies, uint32_t npol, int origin, int device,
                            kw_packed* out, uint32_t chunk_rows) {
  return kw::validate_host_packed(env, b, policies, npol, origin, device, out, chunk_rows);
}

int kw_packed_word(const kw_packed* p, uint64_t row, uint32_t col, uint32_t* word) {
  if (!p || !p->planes || !p->exc_off || !p->dict || (!p->exc && p->exc_count)) return KW_E_ARG;
  return kw::packed_word(p, row, col, word);
}

int kw_packed_unpack(const kw_packed* p, uint64_t row0, uint64_t row1, uint32_t* out) {
  if (!p || !p->exc_off || !p->dict || (p->rows && !p->planes) || (!p->exc && p->exc_count)) return KW_E_ARG;
  return kw::packed_unpack(p, row0, row1, out);
}

int kw_debug_pack_words(const kw_env* env, const int32_t* policies, uint32_t npol, int origin, const uint32_t* words,
                        uint64_t rows, kw_packed* out) {
  if (!env || !out || npol == 0 || out->rows != rows || out->npol != npol || !out->dict) return KW_E_ARG;
  if (!kw::packed_fits(rows, npol)) return KW_E_ARG;
  if (int rc = kw::packed_dict(env->e, policies, npol, origin, out->dict)) return rc;
  return kw::packed_encode(words, out);
}

}  // extern "C"
