// Host check of the data view's definition (csrc/data_view.h), built by tests/test_data_view_host.py
// with the host sanitizers.  Two views hold distinct sentinels in every field (fake addresses, never
// dereferenced).  For each kind of view: one exchange moves exactly the fields the kind brings and no
// other, a second one restores both sides byte for byte; the buffer walk yields every pointer field of
// a view once, and the subset that scs_batch_info counts.  The field table below restates the header
// on purpose: a field added there and not here fails the pointer count.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <set>
#include <type_traits>
#include <vector>

#include "../../selfconcordantsmoothoptimization.jl_amd/csrc/data_view.h"

using namespace scs;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::fprintf(stderr, "FAIL %s at line %d\n", #c, __LINE__); \
      ++fails;                                                    \
    }                                                             \
  } while (0)

// what is exchanged together (the rows of the table in DESIGN §2f)
enum Group { ROWS, WORK, SAMPLE, ROWCOPY, COLCOPY, CSR, SGRAM, VALTYPE, NGROUPS };

#define BLK(G, b) X(G, b.shift) X(G, b.nblk) X(G, b.kp) X(G, b.nnz) X(G, b.ptr) X(G, b.lidx) X(G, b.val)
#define FIELDS                                                                                             \
  X(ROWS, sparse) X(ROWS, A) X(ROWS, a32) X(ROWS, y) X(ROWS, N) X(ROWS, Npad) X(ROWS, nstage) X(ROWS, Nglob) \
  X(WORK, nsplit) X(WORK, nval) X(WORK, nchunk) X(WORK, zpart) X(WORK, z) X(WORK, gN) X(WORK, hN) X(WORK, wN) \
  X(WORK, vN) X(WORK, valpart) X(WORK, tpart)                                                              \
  X(SAMPLE, At) X(SAMPLE, stiles) X(SAMPLE, nstiles) X(SAMPLE, ss.N) X(SAMPLE, ss.NpS) X(SAMPLE, ss.n1pad)  \
  X(SAMPLE, ss.Ps) X(SAMPLE, ss.Ms) X(SAMPLE, ss.bS) X(SAMPLE, ss.uN) X(SAMPLE, ss.hvec) X(SAMPLE, ss.hg)   \
  X(ROWCOPY, nnz) BLK(ROWCOPY, bcsr) BLK(COLCOPY, bcsc)                                                    \
  X(CSR, rowptr) X(CSR, colidx) X(CSR, val) BLK(SGRAM, sgram) X(VALTYPE, sp_f32)

struct Field {
  Group g;
  const char* name;
  bool pointer;
  uint64_t value;
  const void* addr;
};

template <class T>
static uint64_t as_u64(T v) {
  if constexpr (std::is_pointer<T>::value)
    return (uint64_t)(uintptr_t)v;
  else
    return (uint64_t)v;
}

template <class View>
static std::vector<Field> fields(const View& v) {
  std::vector<Field> out;
#define X(G, f) out.push_back({G, #f, std::is_pointer<decltype(v.f)>::value, as_u64(v.f), (const void*)&v.f});
  FIELDS
#undef X
  return out;
}

// sentinel k of side s (0 / 1): distinct over both sides (a bool can only tell the sides apart)
template <class T>
static T sentinel(int k, int s) {
  if constexpr (std::is_same<T, bool>::value)
    return s != 0;
  else if constexpr (std::is_pointer<T>::value)
    return (T)(uintptr_t)(((uint64_t)(s + 1) << 32) + 64u * (unsigned)(k + 1));
  else
    return (T)(1000 * (s + 1) + k);
}

static void fill(ViewData& v, int s) {
  int k = 0;
#define X(G, f) v.f = sentinel<std::remove_reference<decltype(v.f)>::type>(k++, s);
  FIELDS
#undef X
}

// the context's side: the view in place, followed by state that no exchange may touch
struct InPlace : ViewData {
  uint64_t after = 0x0123456789abcdefull;
};

struct Kind {
  const char* name;
  unsigned parts;
  bool moves[NGROUPS];
};

static const Kind KINDS[] = {
    //                                       ROWS  WORK  SAMPLE ROWCOPY COLCOPY CSR  SGRAM VALTYPE
    {"dense", VIEW_DENSE, {true, true, true, false, false, false, false, false}},
    {"sparse batch", VIEW_SPARSE, {true, true, true, true, true, false, false, false}},
    {"sparse batch, sample space", VIEW_SPARSE_SAMPLE, {true, true, true, true, true, true, true, false}},
    {"held-out", VIEW_TEST, {true, true, true, true, false, true, false, true}},
};

static void check_exchange(const Kind& kd) {
  const int fails0 = fails;
  InPlace c;
  NView v;
  // (deterministic padding, so that "byte for byte" below means something)
  std::memset((void*)&c, 0xA5, sizeof c);
  std::memset((void*)&v, 0x5A, sizeof v);
  new (&c) InPlace();
  new (&v) NView();
  fill(c, 0);
  fill(v, 1);
  v.parts = kd.parts;
  unsigned char c0[sizeof c], v0[sizeof v];
  std::memcpy(c0, &c, sizeof c);
  std::memcpy(v0, &v, sizeof v);
  const std::vector<Field> fc = fields(c), fv = fields(v);

  swap_view_data(c, v, v.parts);
  const std::vector<Field> gc = fields(c), gv = fields(v);
  for (size_t i = 0; i < fc.size(); ++i) {
    const bool moved = kd.moves[fc[i].g];
    const bool ok = moved ? (gc[i].value == fv[i].value && gv[i].value == fc[i].value)
                          : (gc[i].value == fc[i].value && gv[i].value == fv[i].value);
    if (!ok) {
      std::fprintf(stderr, "FAIL %s: field %s %s\n", kd.name, fc[i].name, moved ? "was not exchanged" : "was touched");
      ++fails;
    }
    CHECK(fc[i].value != fv[i].value);   // the sentinels tell the sides apart
  }
  CHECK(v.parts == kd.parts);
  CHECK(c.after == 0x0123456789abcdefull);

  swap_view_data(c, v, v.parts);
  CHECK(std::memcmp(c0, &c, sizeof c) == 0);
  CHECK(std::memcmp(v0, &v, sizeof v) == 0);
  std::printf("exchange %-28s %s\n", kd.name, fails == fails0 ? "ok" : "FAILED");
}

static void check_buffers() {
  NView v;
  fill(v, 1);
  const std::vector<Field> f = fields(v);
  std::set<const void*> pointer_fields, counted;
  for (const Field& x : f)
    if (x.pointer) {
      pointer_fields.insert(x.addr);
      // y, the N-space workspace, bcsr, bcsc, the CSR and sgram: not A, not the sample space
      if (x.g != SAMPLE && std::strcmp(x.name, "A") != 0) counted.insert(x.addr);
    }
  CHECK(pointer_fields.size() == 30);

  std::vector<const void*> got;
  std::set<uint64_t> values;
  view_buffers(v, VB_ALL, [&](auto*& p) {
    got.push_back((const void*)&p);
    values.insert(as_u64(p));
  });
  CHECK(got.size() == pointer_fields.size());
  CHECK(std::set<const void*>(got.begin(), got.end()) == pointer_fields);   // every one, once
  CHECK(values.size() == got.size());                                       // each address distinct

  // a const view walks by value (sparse_view_bytes)
  const NView& cv = v;
  std::set<uint64_t> sub, want;
  size_t n = 0;
  view_buffers(cv, VB_SPARSE_VIEW, [&](const void* p) {
    sub.insert((uint64_t)(uintptr_t)p);
    ++n;
  });
  for (const Field& x : f)
    if (counted.count(x.addr)) want.insert(x.value);
  CHECK(n == counted.size() && sub == want);

  // the groups are disjoint and cover VB_ALL
  size_t total = 0;
  for (unsigned g = 1; g <= VB_ALL; g <<= 1) view_buffers(cv, g, [&](const void*) { ++total; });
  CHECK(total == pointer_fields.size());
  std::printf("buffers %zu, counted as a sparse view's bytes %zu\n", got.size(), n);
}

int main() {
  for (const Kind& kd : KINDS) check_exchange(kd);
  check_buffers();
  if (fails) std::fprintf(stderr, "%d check(s) failed\n", fails);
  return fails ? 1 : 0;
}
