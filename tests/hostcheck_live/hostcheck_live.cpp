// TEST-ONLY: xcd_map.h (where the kernels launched per pair and chunk place their workgroups) compiled for the host behind
// extern "C" wrappers, for tests/test_live_map_hostcheck.py. With -DHOSTCHECK_LIVE_MAIN the file is a stand-alone program
// that walks generated grids through the same wrappers (the `san` target builds it with -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../loam_amd/csrc/xcd_map.h"

using namespace loamx;

extern "C" {

// workgroups 0 .. n_blocks - 1 of a grid through xcd_live_map: ok[b] = its return value, pair[b] / chunk[b] what it gave
// (0xFFFFFFFF where it returned false)
void hostcheck_live_walk(uint32_t n_blocks, uint32_t blocks_per_pair, uint64_t n_pairs, uint32_t n_live, const uint32_t* live, uint8_t* ok,
                         uint32_t* pair, uint32_t* chunk) {
  for (uint32_t b = 0; b < n_blocks; b++) {
    size_t p = 0;
    uint32_t c = 0;
    ok[b] = xcd_live_map(b, blocks_per_pair, (size_t)n_pairs, n_live, live, p, c) ? 1 : 0;
    pair[b] = ok[b] ? (uint32_t)p : 0xFFFFFFFFu, chunk[b] = ok[b] ? c : 0xFFFFFFFFu;
  }
}

// the same through xcd_pair_map
void hostcheck_pair_walk(uint32_t n_blocks, uint32_t blocks_per_pair, uint64_t n_pairs, uint8_t* ok, uint32_t* pair, uint32_t* chunk) {
  for (uint32_t b = 0; b < n_blocks; b++) {
    size_t p = 0;
    uint32_t c = 0;
    ok[b] = xcd_pair_map(b, blocks_per_pair, (size_t)n_pairs, p, c) ? 1 : 0;
    pair[b] = ok[b] ? (uint32_t)p : 0xFFFFFFFFu, chunk[b] = ok[b] ? c : 0xFFFFFFFFu;
  }
}

}  // extern "C"

#ifdef HOSTCHECK_LIVE_MAIN
int main() {
  uint64_t state = 88172645463325252ull, walked = 0;
  auto rnd = [&]() {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return state >> 11;
  };
  for (uint64_t n_pairs = 8; n_pairs <= 40; n_pairs++)
    for (uint32_t bpp : {1u, 2u, 5u, 77u})
      for (int rep = 0; rep < 4; rep++) {
        std::vector<uint32_t> live;  // exactly as long as the list: a read past n_live is a heap overflow
        for (uint32_t p = 0; p < n_pairs; p++)
          if (rep == 3 || (rep > 0 && rnd() % 3 != 0)) live.push_back(p);
        const uint32_t n_blocks = (uint32_t)((n_pairs + 7) / 8 * 8 * bpp) + 16 * bpp;  // (the grid and two lanes' worth past it)
        std::vector<uint8_t> ok(n_blocks);
        std::vector<uint32_t> pair(n_blocks), chunk(n_blocks);
        hostcheck_live_walk(n_blocks, bpp, n_pairs, (uint32_t)live.size(), live.data(), ok.data(), pair.data(), chunk.data());
        uint64_t produced = 0;
        for (uint32_t b = 0; b < n_blocks; b++) produced += ok[b];
        if (produced != live.size() * bpp) {
          printf("n_pairs %llu blocks_per_pair %u: %llu workgroups with work, want %llu\n", (unsigned long long)n_pairs, bpp,
                 (unsigned long long)produced, (unsigned long long)(live.size() * bpp));
          return 1;
        }
        hostcheck_pair_walk(n_blocks, bpp, n_pairs, ok.data(), pair.data(), chunk.data());
        walked += 2 * n_blocks;
      }
  printf("hostcheck_live ok: %llu workgroups\n", (unsigned long long)walked);
  return 0;
}
#endif
