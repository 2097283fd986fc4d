// Host check of the sparse batch views' bookkeeping (csrc/batch_plan.h), built by
// tests/test_sparse_batches_host.py with the host sanitizers.  Replays cyclic epochs over a batch list
// the way scs_select_batch drives the plan (find, else refill_target + place) and prints one line per
// scenario: "budget nbatch epochs builds nslots kept_bytes total_bytes : slot-of-each-batch-or--1 ..."
// for the Python side to compare with its own statement of the rule.  Exits non-zero if a structural
// property fails.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../selfconcordantsmoothoptimization.jl_amd/csrc/batch_plan.h"

using namespace scs;

static int fails = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "FAIL %s at line %d\n", #c, __LINE__);      \
      ++fails;                                                         \
    }                                                                  \
  } while (0)

struct Batch {
  long long n, bytes;
};

static void replay(long long budget, const std::vector<Batch>& bs, int epochs) {
  BatchPlan p;
  p.reset(budget);
  CHECK(p.slots.empty() && p.builds == 0 && p.kept_bytes == 0);
  for (int e = 0; e < epochs; ++e)
    for (size_t b = 0; b < bs.size(); ++b) {
      int k = p.find((int64_t)b);
      if (k < 0) {
        const int t = p.refill_target(bs[b].n, bs[b].n, bs[b].bytes);
        if (t >= 0) {   // the caller frees the old view first
          CHECK(!p.slots[t].kept && p.slots[t].n == bs[b].n);
          p.slots[t].batch = -1;
          p.slots[t].bytes = 0;
        }
        bool fresh = false;
        const size_t before = p.slots.size();
        k = p.place((int64_t)b, bs[b].n, bs[b].n, bs[b].bytes, &fresh);
        CHECK(fresh == (t < 0) && (fresh ? (size_t)k == before : k == t));
        CHECK(p.slots.size() == before + (fresh ? 1 : 0));
      }
      CHECK(k >= 0 && k < (int)p.slots.size() && p.slots[k].batch == (int64_t)b && p.slots[k].bytes == bs[b].bytes);
      // the kept views stay within the budget, a kept view is never replaced, one refillable slot per size
      int64_t kept = 0;
      for (size_t i = 0; i < p.slots.size(); ++i) {
        if (p.slots[i].kept) kept += p.slots[i].bytes;
        for (size_t j = i + 1; j < p.slots.size(); ++j) {
          CHECK(p.slots[i].batch < 0 || p.slots[i].batch != p.slots[j].batch);
          CHECK(p.slots[i].kept || p.slots[j].kept || p.slots[i].n != p.slots[j].n);
        }
      }
      CHECK(kept == p.kept_bytes && kept <= p.budget);
    }
  std::printf("%lld %zu %d %lld %zu %lld %lld :", budget, bs.size(), epochs, (long long)p.builds, p.slots.size(),
              (long long)p.kept_bytes, (long long)p.total_bytes());
  for (size_t b = 0; b < bs.size(); ++b) std::printf(" %d", p.find((int64_t)b));
  std::printf("\n");
}

int main() {
  const std::vector<Batch> loader = {{400, 1000}, {400, 1010}, {400, 990}, {300, 800}};   // a partial last batch
  std::vector<Batch> slices;                                                             // slice_samples: one-row batches
  for (int i = 0; i < 40; ++i) slices.push_back({1, 8 * 96 + 64});
  const std::vector<Batch> mixed = {{64, 500}, {65, 500}, {64, 700}, {1, 100}, {65, 100}, {1, 100}, {64, 10}};
  const long long budgets[] = {0, 1, 999, 1000, 2010, 3000, 3799, 3800, 1000000, INT64_MAX};
  for (long long bud : budgets)
    for (int ep : {1, 2, 3}) {
      replay(bud, loader, ep);
      replay(bud, slices, ep);
      replay(bud, mixed, ep);
    }
  // the budget's text form
  CHECK(batch_budget_bytes(nullptr, 77) == 77 && batch_budget_bytes("", 77) == 77 && batch_budget_bytes("x", 77) == 77);
  CHECK(batch_budget_bytes("-1", 77) == 77 && batch_budget_bytes("nan", 77) == 77);
  CHECK(batch_budget_bytes("0", 77) == 0 && batch_budget_bytes("1", 77) == 1048576);
  CHECK(batch_budget_bytes("0.5", 77) == 524288 && batch_budget_bytes("1e30", 77) == INT64_MAX);
  CHECK(batch_budget_bytes("inf", 77) == INT64_MAX && batch_budget_bytes("8796093022207", 77) == INT64_MAX);
  BatchPlan neg;
  neg.reset(-5);   // a negative budget keeps nothing
  CHECK(neg.budget == 0);
  return fails ? 1 : 0;
}
