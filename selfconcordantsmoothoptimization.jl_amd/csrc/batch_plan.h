// Host-only bookkeeping of the sparse minibatch views (scs_set_sparse_batches): which batch each
// view holds, which views are kept and which slot a new view goes to.  Pure C++ (no HIP), so
// tests/test_sparse_batches_host.py compiles it with the host sanitizers and checks it without a GPU.
//
// Building a view costs far more than a product on it, so views are kept per batch, in the order
// built, while their bytes stay within a budget.  A kept view is never evicted: with the loader's
// cyclic batch order an LRU rule would evict every view just before its next use.  A batch whose
// view does not fit shares one refillable slot with the other such batches of its (local, global)
// size, as the dense pool does.
#pragma once
#include <stdint.h>

#include <cstdlib>
#include <vector>

namespace scs {

struct BatchSlot {
  int64_t n = 0, nglob = 0;   // local and global rows of the batches this slot serves
  int64_t batch = -1;         // the batch it holds
  int64_t bytes = 0;          // device bytes of its view
  bool kept = false;          // kept for `batch` (false: refillable)
};

struct BatchPlan {
  int64_t budget = 0;       // bytes the kept views may take together
  int64_t kept_bytes = 0;
  int64_t builds = 0;       // views built since reset()
  std::vector<BatchSlot> slots;

  void reset(int64_t budget_bytes) {
    budget = budget_bytes < 0 ? 0 : budget_bytes;
    kept_bytes = 0;
    builds = 0;
    slots.clear();
  }

  // the slot whose view holds batch b (-1: none)
  int find(int64_t b) const {
    for (int i = 0; i < (int)slots.size(); ++i)
      if (slots[i].batch == b) return i;
    return -1;
  }

  // the existing refillable slot that place() would refill with a view of these sizes (-1: place()
  // appends a slot): its old view can be freed before the new one is allocated
  int refill_target(int64_t n, int64_t nglob, int64_t bytes) const {
    if (bytes <= budget - kept_bytes) return -1;
    for (int i = 0; i < (int)slots.size(); ++i)
      if (!slots[i].kept && slots[i].n == n && slots[i].nglob == nglob) return i;
    return -1;
  }

  // The slot of the newly sized view of batch b (`bytes` > 0 device bytes, never held before this
  // call): a new kept slot while the budget lasts, else the refillable slot of its size -- an
  // existing one (*fresh = false: its view is replaced) or a new one.  Counts one build.
  int place(int64_t b, int64_t n, int64_t nglob, int64_t bytes, bool* fresh) {
    ++builds;
    BatchSlot s;
    s.n = n;
    s.nglob = nglob;
    s.batch = b;
    s.bytes = bytes;
    if (bytes <= budget - kept_bytes) {   // budget >= kept_bytes always: no overflow
      s.kept = true;
      kept_bytes += bytes;
      slots.push_back(s);
      *fresh = true;
      return (int)slots.size() - 1;
    }
    for (int i = 0; i < (int)slots.size(); ++i)
      if (!slots[i].kept && slots[i].n == n && slots[i].nglob == nglob) {
        slots[i] = s;
        *fresh = false;
        return i;
      }
    slots.push_back(s);
    *fresh = true;
    return (int)slots.size() - 1;
  }

  int64_t total_bytes() const {
    int64_t t = 0;
    for (const BatchSlot& s : slots) t += s.bytes;
    return t;
  }
};

// SCS_SPARSE_BATCH_CACHE_MB as the budget in bytes: `text` null, empty or not a non-negative number
// gives `dflt` (the bytes the context's sparse data takes); values past 2^43 MB saturate.
inline int64_t batch_budget_bytes(const char* text, int64_t dflt) {
  if (!text || !*text) return dflt;
  char* end = nullptr;
  const double mb = std::strtod(text, &end);
  if (end == text || !(mb >= 0.0)) return dflt;
  if (mb >= 8796093022207.0) return INT64_MAX;   // 2^43 MB = 2^63 bytes
  return (int64_t)(mb * 1048576.0);
}

}  // namespace scs
