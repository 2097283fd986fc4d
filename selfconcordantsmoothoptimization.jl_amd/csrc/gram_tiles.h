// The 256 x 128 tile list of the main Gram and the decoding of its items, in plain C++ (the kernels,
// the host setup and tests/native/gram_tiles_check.cpp share this one definition).
//
// A list item (x, y) -- the int2 of the plain list, the first two fields of an int4 work item and
// of a combine item -- is one of
//   y >= 0: tile (I, bj) = (x, y): rows = 128-blocks 2I, 2I+1, column panel bj (bj <= 2I+1);
//   y <  0: a pair tile of row blocks I = x and I' = -1 - y: rows 0..127 are the diagonal block
//           D1(I) = (2I+1, 2I+1), rows 128..255 are D1(I') = (2I'+1, 2I'+1).
// The tile (I, 2I+1) = [U; D1(I)] of the unpaired list computes, in its upper half, the mirror U of
// the block L that tile (I, 2I) = [D0; L] already holds; a pair tile does the D1 halves of two such
// tiles and no U.  With an odd number of row blocks the last one keeps its [U; D1] tile.
#pragma once

#if defined(__HIPCC__)
#define SCS_TILES_HD __host__ __device__
#else
#define SCS_TILES_HD
#endif

namespace scs {

SCS_TILES_HD inline bool gram_item_is_pair(int y) { return y < 0; }
SCS_TILES_HD inline int gram_pair_encode(int I2) { return -1 - I2; }
SCS_TILES_HD inline int gram_pair_second(int y) { return -1 - y; }

// The two 128-row panels of A that form the rows of a 256 x 128 item (its A1 operand).
SCS_TILES_HD inline void gram_item_panels(int x, int y, int* pa, int* pb) {
  if (gram_item_is_pair(y)) {
    *pa = 2 * x + 1;
    *pb = 2 * gram_pair_second(y) + 1;
  } else {
    *pa = 2 * x;
    *pb = 2 * x + 1;
  }
}

// The 128 x 128 block (row block, column block) that rows 128 h .. 128 h + 127 (h = 0, 1) of a
// 256 x 128 item hold.
SCS_TILES_HD inline void gram_item_block(int x, int y, int h, int* bi, int* bj) {
  if (gram_item_is_pair(y)) {
    *bi = *bj = 2 * (h ? gram_pair_second(y) : x) + 1;
  } else {
    *bi = 2 * x + h;
    *bj = y;
  }
}

// Whether an AV launch gives this item the fused Aᵀv of its column panel(s): the tile whose row
// block holds its column panel (gti = tile rows, 128 or 256), and every pair tile (both panels).
SCS_TILES_HD inline bool gram_item_designated(int x, int y, int gti) {
  return gram_item_is_pair(y) || x == (int)((long long)y * 128 / gti);
}

// Super-blocked list of 256 x 128 tiles for the TI = 4 kernels: row block I covers 128-blocks 2I,
// 2I+1; every tile with bj <= 2I+1.  nb even.  pair: the tiles (I, 2I+1) of row blocks I = 2k and
// 2k+1 (the same super-block of 4) become one pair item at the place of the first.  make(x, y)
// builds the caller's item type.  Returns the number of items: sum(2I+2), less nb/4 when paired.
template <class T2, class Make>
inline int gram_tile_list_tall_t(int nb, bool pair, T2* out, Make make) {
  const int nbi = nb / 2, SI = 4, SJ = 8;
  int t = 0;
  for (int sbi = 0; sbi < (nbi + SI - 1) / SI; ++sbi)
    for (int sbj = 0; sbj <= sbi; ++sbj)
      for (int I = sbi * SI; I < (sbi + 1) * SI && I < nbi; ++I)
        for (int j = sbj * SJ; j < (sbj + 1) * SJ && j < nb; ++j) {
          if (j > 2 * I + 1) continue;
          if (pair && j == 2 * I + 1) {
            if (I % 2 == 1) continue;   // in the pair item of I - 1
            if (I + 1 < nbi) {
              out[t++] = make(I, gram_pair_encode(I + 1));
              continue;
            }
          }
          out[t++] = make(I, j);
        }
  return t;
}

}  // namespace scs
