// The Punkt tables of a context: lddl_punkt_set_params parses the caller's two blobs on the host
// (punkt_params.h), uploads them and swaps them in for the ones before; segment.hip and bart.hip
// read them. Launches no kernel.
#include <hip/hip_runtime.h>

#include "common.h"
#include "ctx.h"
#include "lddl_amd.h"
#include "punkt_params.h"
#include "punkt_state.h"

using namespace lddl;

namespace {

void free_tables(PunktTab& t) {
  for (const void* p : {(const void*)t.cls.l1, (const void*)t.cls.pages, (const void*)t.lower,
                        (const void*)t.hash, (const void*)t.keys})
    (void)hipFree(const_cast<void*>(p));
  t = PunktTab{};
}

int upload_tables(const PunktClassBlob& cb, const PunktParamTable& pt, PunktTab* t) {
  int rc;
  if ((rc = upload(&t->cls.l1, cb.l1, kPunktL1Bytes)) ||
      (rc = upload(&t->cls.pages, cb.pages, (size_t)cb.n_pages * 256)) ||
      (rc = upload(&t->lower, cb.lower, (size_t)cb.n_lower * 8)) ||
      (rc = upload(&t->hash, pt.hash.data(), sizeof(PkEnt) * pt.hash.size())) ||
      (rc = upload(&t->keys, pt.keys.data(), pt.keys.size())))
    return rc;
  t->n_lower = (int32_t)cb.n_lower;
  t->hmask = pt.hmask;
  t->n_rec = pt.n_ent;
  LDDL_HIP(hipDeviceSynchronize());  // nothing on the device reads the tables before these any more
  return 0;
}

}  // namespace

bool lddl::punkt_class_tab(const lddl_ctx* c, ClassTab* out) {
  if (!c->punkt || !c->punkt->tab.cls.l1) return false;
  *out = c->punkt->tab.cls;
  return true;
}

extern "C" void lddl_punkt_release(lddl_ctx* c) {
  if (!c->punkt) return;
  (void)hipDeviceSynchronize();
  free_tables(c->punkt->tab);
  delete c->punkt;  // (a pending segmentation's blocks go back to the arena)
  c->punkt = nullptr;
}

extern "C" int lddl_punkt_set_params(lddl_ctx* c, const uint8_t* table, int64_t table_bytes,
                                     const uint8_t* records, int64_t records_bytes) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  PunktClassBlob cb;
  PunktParamTable pt;
  int rc;
  if ((rc = parse_punkt_table(table, table_bytes, &cb)) ||
      (rc = parse_punkt_records(records, records_bytes, &pt)))
    return rc;
  LDDL_HIP(hipSetDevice(c->device));
  PunktTab fresh{};
  if ((rc = upload_tables(cb, pt, &fresh)) == 0) {  // swap them in; what goes out is freed below
    if (!c->punkt) c->punkt = new lddl_punkt_state();
    std::swap(c->punkt->tab, fresh);
  }
  free_tables(fresh);
  return rc;
}
