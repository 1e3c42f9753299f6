// CPU check of the host side of lddl_punkt_set_params (csrc/punkt_params.h): the shipped
// character class table and the golden parameter records parse, every record is found with its
// value, and every refusal comes with its message. Built with AddressSanitizer + UBSan together
// with csrc/errors.cpp by tests/test_punkt_params.py, which passes the two files; exits non-zero
// on the first failed expectation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "lddl_amd.h"
#include "punkt_params.h"

using namespace lddl;
typedef std::vector<uint8_t> Bytes;

#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static Bytes read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  EXPECT(f.good());
  return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// the blob handed over in an exact-size heap block, so that ASan sees any read past its end
static int table_rc(const Bytes& b, PunktClassBlob* out = nullptr) {
  PunktClassBlob cb;
  Bytes exact(b.begin(), b.end());
  exact.shrink_to_fit();
  return parse_punkt_table(exact.empty() ? nullptr : exact.data(), (int64_t)exact.size(), out ? out : &cb);
}
static int records_rc(const Bytes& b, PunktParamTable* out = nullptr) {
  PunktParamTable pt;
  Bytes exact(b.begin(), b.end());
  exact.shrink_to_fit();
  // (an empty blob still comes with a pointer, as lddl_amd/punkt.py passes it)
  static const uint8_t none[1] = {0};
  return parse_punkt_records(exact.empty() ? none : exact.data(), (int64_t)exact.size(), out ? out : &pt);
}
static bool refused(int rc, const std::string& msg) { return rc == -1 && msg == lddl_last_error(); }

static Bytes record(int kind, int value, const std::string& a, const std::string& b = "", int la = -1,
                    int lb = -1) {
  if (la < 0) la = (int)a.size();
  if (lb < 0) lb = (int)b.size();
  Bytes r = {(uint8_t)kind, (uint8_t)value, (uint8_t)(la & 255), (uint8_t)(la >> 8), (uint8_t)(lb & 255),
             (uint8_t)(lb >> 8)};
  r.insert(r.end(), a.begin(), a.end());
  r.insert(r.end(), b.begin(), b.end());
  return r;
}
static Bytes operator+(Bytes a, const Bytes& b) {
  a.insert(a.end(), b.begin(), b.end());
  return a;
}

static int find(const PunktParamTable& t, uint32_t kind, const std::string& a, const std::string& b = "") {
  return find_param(t.hash.data(), t.hmask, t.keys.data(), kind, (const uint8_t*)a.data(), (int)a.size(),
                    (const uint8_t*)b.data(), (int)b.size());
}

static void put_u32(Bytes& b, size_t at, uint32_t v) { memcpy(b.data() + at, &v, 4); }
static void put_u16(Bytes& b, size_t at, uint16_t v) { memcpy(b.data() + at, &v, 2); }

int main(int argc, char** argv) {
  EXPECT(argc == 3);  // punkt_props.bin, the golden parameters' records
  const Bytes table = read_file(argv[1]), recs = read_file(argv[2]);

  // ---- the shipped class table ----
  PunktClassBlob cb;
  EXPECT(table_rc(table, &cb) == 0);
  uint32_t hdr[3];
  memcpy(hdr, table.data() + 4, 12);
  EXPECT(cb.n_pages == hdr[1] && cb.n_lower == hdr[2] && cb.n_pages > 0 && cb.n_lower > 0);
  const int64_t need = 16 + kPunktL1Bytes + (int64_t)cb.n_pages * 256 + (int64_t)cb.n_lower * 8;
  EXPECT((int64_t)table.size() == need);
  {  // a table that is exactly `need` long inside a longer buffer parses the same
    Bytes longer = table;
    longer.resize(table.size() + 7, 0xEE);
    PunktClassBlob c2;
    EXPECT(table_rc(longer, &c2) == 0 && c2.n_pages == cb.n_pages && c2.n_lower == cb.n_lower);
  }
  // ---- its refusals ----
  {
    Bytes t = table;
    t[0] = 'X';
    EXPECT(refused(table_rc(t), "bad Punkt character table"));
    EXPECT(refused(table_rc(Bytes()), "bad Punkt character table"));
    EXPECT(refused(table_rc(Bytes(table.begin(), table.begin() + 16 + kPunktL1Bytes - 1)),
                   "bad Punkt character table"));
    t = table;
    for (uint32_t v : {0u, 2u}) {
      put_u32(t, 4, v);
      EXPECT(refused(table_rc(t), "truncated Punkt character table"));
    }
    EXPECT(refused(table_rc(Bytes(table.begin(), table.end() - 1)), "truncated Punkt character table"));
    EXPECT(refused(table_rc(Bytes(table.begin(), table.begin() + 16 + kPunktL1Bytes)),
                   "truncated Punkt character table"));
    // an l1 entry equal to the page count (first, middle and last entry)
    for (int i : {0, 0x123, 0x10FF}) {
      t = table;
      put_u16(t, 16 + 2 * (size_t)i, (uint16_t)cb.n_pages);
      char msg[128];
      snprintf(msg, sizeof msg, "Punkt character table: l1[%d] names a page past the last of %u", i,
               cb.n_pages);
      EXPECT(refused(table_rc(t), msg));
      put_u16(t, 16 + 2 * (size_t)i, (uint16_t)(cb.n_pages - 1));
      EXPECT(table_rc(t) == 0);
    }
    // lower_cp bisects the (cp, lower) pairs: equal and descending neighbours are refused
    const size_t low = 16 + kPunktL1Bytes + (size_t)cb.n_pages * 256;
    uint32_t cp0;
    memcpy(&cp0, table.data() + low, 4);
    t = table;
    put_u32(t, low + 8, cp0);
    EXPECT(refused(table_rc(t), "Punkt character table: lowercase pairs not ascending at 1"));
    t = table;
    put_u32(t, low + 8 * (size_t)(cb.n_lower - 1), 0);
    char msg[128];
    snprintf(msg, sizeof msg, "Punkt character table: lowercase pairs not ascending at %u", cb.n_lower - 1);
    EXPECT(refused(table_rc(t), msg));
  }

  // ---- the golden records: every one is found with its value ----
  PunktParamTable pt;
  EXPECT(records_rc(recs, &pt) == 0);
  std::set<std::tuple<int, std::string, std::string>> distinct;
  size_t n_rec = 0;
  for (size_t r = 0; r < recs.size(); ++n_rec) {
    const int kind = recs[r], value = recs[r + 1];
    const int la = recs[r + 2] | (recs[r + 3] << 8), lb = recs[r + 4] | (recs[r + 5] << 8);
    const std::string a(recs.begin() + r + 6, recs.begin() + r + 6 + la);
    const std::string b(recs.begin() + r + 6 + la, recs.begin() + r + 6 + la + lb);
    // (the writer emits each key once, so the value of a record is the first of its key)
    EXPECT(distinct.insert(std::make_tuple(kind, a, b)).second);
    EXPECT(find(pt, (uint32_t)kind, a, b) == value);
    r += 6 + (size_t)la + (size_t)lb;
  }
  EXPECT(pt.n_ent == (int32_t)distinct.size() && n_rec == distinct.size());
  for (int kind = 1; kind <= 4; ++kind) {  // the golden parameters have records of every kind
    bool any = false;
    for (const auto& k : distinct) any |= std::get<0>(k) == kind;
    EXPECT(any);
  }
  EXPECT(pt.hash.size() == (size_t)pt.hmask + 1 && (pt.hash.size() & pt.hmask) == 0);
  EXPECT(pt.hash.size() >= 2 * n_rec + 16 && pt.hash.size() < 2 * (2 * n_rec + 16));
  size_t used = 0;
  for (const PkEnt& e : pt.hash) used += e.kind != 0;
  EXPECT(used == distinct.size());
  // absent keys: another kind, a prefix, an extension, a collocation's halves swapped or alone
  for (const auto& k : distinct) {
    const int kind = std::get<0>(k);
    const std::string &a = std::get<1>(k), &b = std::get<2>(k);
    if (!distinct.count(std::make_tuple(kind, a + "~", b))) EXPECT(find(pt, kind, a + "~", b) == -1);
    if (!a.empty() && !distinct.count(std::make_tuple(kind, a.substr(0, a.size() - 1), b)))
      EXPECT(find(pt, kind, a.substr(0, a.size() - 1), b) == -1);
    const int other = kind % 3 + 1;  // of the three one-key kinds
    if (kind != 4 && !distinct.count(std::make_tuple(other, a, std::string()))) EXPECT(find(pt, other, a) == -1);
    if (kind == 4 && a != b && !distinct.count(std::make_tuple(4, b, a))) EXPECT(find(pt, 4, b, a) == -1);
    if (kind == 4 && !b.empty() && !distinct.count(std::make_tuple(4, a, std::string())))
      EXPECT(find(pt, 4, a, "") == -1);
  }
  EXPECT(find(pt, kKAbbrev, "no such abbreviation in any model") == -1);
  EXPECT(find(pt, kKAbbrev, "") == -1);

  // ---- no records: an empty table of 16 slots, in which nothing is found ----
  {
    PunktParamTable e;
    EXPECT(records_rc(Bytes(), &e) == 0);
    EXPECT(e.hash.size() == 16 && e.hmask == 15 && e.n_ent == 0 && e.keys.empty());
    for (const PkEnt& x : e.hash) EXPECT(x.kind == 0);
    EXPECT(find(e, kKAbbrev, "dr") == -1 && find(e, kKColloc, "a", "b") == -1);
    PunktParamTable z;
    EXPECT(parse_punkt_records(nullptr, 0, &z) == 0 && z.hash.size() == 16 && z.n_ent == 0);
  }
  // ---- a record sent twice is stored once; the first value wins ----
  {
    PunktParamTable d;
    EXPECT(records_rc(record(3, 34, "word") + record(1, 0, "dr") + record(3, 66, "word") +
                          record(4, 0, "a", "b") + record(4, 0, "a", "b") + record(4, 0, "ab", "") +
                          record(1, 0, "") + record(1, 0, ""),
                      &d) == 0);
    EXPECT(d.n_ent == 5 && d.hash.size() == 32);
    EXPECT(find(d, 3, "word") == 34 && find(d, 1, "dr") == 0 && find(d, 4, "a", "b") == 0);
    EXPECT(find(d, 4, "ab", "") == 0 && find(d, 4, "", "ab") == -1 && find(d, 4, "b", "a") == -1);
    EXPECT(find(d, 1, "") == 0 && find(d, 2, "") == -1 && find(d, 1, "word") == -1);
  }
  // ---- the records' refusals ----
  {
    const Bytes ok = record(1, 0, "dr"), two = ok + record(4, 0, "a", "b");
    EXPECT(records_rc(two) == 0);
    EXPECT(refused(records_rc(Bytes(two.begin(), two.begin() + ok.size() + 5)),
                   "truncated Punkt parameter record"));
    EXPECT(refused(records_rc(Bytes(ok.begin(), ok.begin() + 5)), "truncated Punkt parameter record"));
    EXPECT(refused(records_rc(Bytes(two.begin(), two.end() - 1)), "truncated Punkt parameter record"));
    EXPECT(refused(records_rc(ok + record(4, 0, "a", "b", 1, 2)), "truncated Punkt parameter record"));
    EXPECT(refused(records_rc(ok + record(1, 0, "a", "", 2)), "truncated Punkt parameter record"));
    EXPECT(refused(records_rc(ok + record(0, 0, "x")), "bad Punkt parameter kind 0"));
    EXPECT(refused(records_rc(record(5, 0, "x") + ok), "bad Punkt parameter kind 5"));
    const std::string k255(255, 'k'), k256(256, 'k');
    PunktParamTable p;
    EXPECT(records_rc(record(1, 0, k255) + record(4, 7, k255, k255), &p) == 0);
    EXPECT(find(p, 1, k255) == 0 && find(p, 4, k255, k255) == 7);
    EXPECT(refused(records_rc(record(1, 0, k256)), "Punkt parameter key longer than 255 bytes"));
    EXPECT(refused(records_rc(record(4, 0, "a", k256)), "Punkt parameter key longer than 255 bytes"));
    PunktParamTable n;
    EXPECT(refused(parse_punkt_records(nullptr, 1, &n), "null Punkt parameter records"));
    EXPECT(refused(parse_punkt_records(nullptr, (int64_t)1 << 40, &n), "null Punkt parameter records"));
  }
  printf("punkt_params_check ok\n");
  return 0;
}
