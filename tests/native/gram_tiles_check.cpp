// Host check of the main Gram's 256 x 128 tile list and its pair items (csrc/gram_tiles.h), built by
// tests/test_gram_tiles.py with the host sanitizers.  For each number of 128-blocks nb: every block
// (i, j) with i >= j is produced by exactly one item half, no block with i < j is produced except
// the one leftover U of an odd number of row blocks, every column panel has exactly one item that
// owns its fused Aᵀv rows, and the item count is sum(2I+2) - floor(nbi / 2).  Prints one line per
// (nb, paired) "nb paired items" and exits non-zero if a property fails.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../selfconcordantsmoothoptimization.jl_amd/csrc/gram_tiles.h"

using namespace scs;

static int fails = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "FAIL %s at line %d\n", #c, __LINE__);      \
      ++fails;                                                         \
    }                                                                  \
  } while (0)

struct Item {
  int x, y;
};

int main() {
  const int nbs[] = {2, 4, 6, 10, 96, 128};
  for (int nb : nbs)
    for (int paired = 0; paired <= 1; ++paired) {
      const int nbi = nb / 2;
      int full = 0;
      for (int I = 0; I < nbi; ++I) full += 2 * I + 2;
      std::vector<Item> tl((size_t)full);   // exactly the unpaired count: an overrun is a sanitizer error
      const int nt = gram_tile_list_tall_t(nb, paired != 0, tl.data(), [](int x, int y) { return Item{x, y}; });
      CHECK(nt == full - (paired ? nbi / 2 : 0));
      std::vector<int> cover((size_t)nb * nb, 0), owner((size_t)nb, 0);
      int npair = 0;
      for (int t = 0; t < nt; ++t) {
        const Item it = tl[(size_t)t];
        CHECK(it.x >= 0 && it.x < nbi);
        int pa, pb;
        gram_item_panels(it.x, it.y, &pa, &pb);
        CHECK(pa >= 0 && pa < nb && pb >= 0 && pb < nb);
        if (gram_item_is_pair(it.y)) {
          ++npair;
          const int I2 = gram_pair_second(it.y);
          CHECK(gram_pair_encode(I2) == it.y);
          CHECK(I2 == it.x + 1 && it.x % 2 == 0 && it.x / 4 == I2 / 4);   // the same super-block of row blocks
          CHECK(gram_item_designated(it.x, it.y, 256));
          ++owner[(size_t)pa];
          ++owner[(size_t)pb];
        } else {
          CHECK(it.y <= 2 * it.x + 1 && it.y < nb);
          if (gram_item_designated(it.x, it.y, 256)) ++owner[(size_t)it.y];
        }
        for (int h = 0; h < 2; ++h) {
          int bi, bj;
          gram_item_block(it.x, it.y, h, &bi, &bj);
          CHECK(bi >= 0 && bi < nb && bj >= 0 && bj < nb);
          CHECK(bi == (h ? pb : pa));   // the rows of half h are the panel the A1 operand loads there
          ++cover[(size_t)bi * nb + bj];
        }
      }
      CHECK(npair == (paired ? nbi / 2 : 0));
      for (int i = 0; i < nb; ++i) {
        CHECK(owner[(size_t)i] == 1);
        for (int j = 0; j < nb; ++j) {
          const int c = cover[(size_t)i * nb + j];
          if (i >= j) CHECK(c == 1);
          else if (j == i + 1 && i % 2 == 0 && (!paired || (nbi % 2 == 1 && i == nb - 2))) CHECK(c == 1);   // a U block
          else CHECK(c == 0);
        }
      }
      std::printf("%d %d %d\n", nb, paired, nt);
    }
  return fails ? 1 : 0;
}
