// TEST-ONLY: crop_math.h (the rule of the map window) compiled for the host as a program of its own, for
// tests/test_crop_hostcheck.py (the file formats: tests/crop_common.py).
//   hostcheck_crop IN OUT   records of a centre, a box, a leaf and a voxel key -> the skip decision, the bounds and the key's decision
// The `san` target builds the same file with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../loam_amd/csrc/crop_math.h"

using namespace loamx;

struct CropIn {
  double c[3], lo[3], hi[3], leaf;
  uint64_t key;
};
struct CropOut {
  uint64_t skip;
  double flo[3], fhi[3];
  uint64_t keep;
};
static_assert(sizeof(CropIn) == 88 && sizeof(CropOut) == 64, "the formats of tests/crop_common.py");

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 1;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<CropIn> in;
  CropIn rec;
  while (fread(&rec, sizeof(rec), 1, f) == 1) in.push_back(rec);
  fclose(f);
  std::vector<CropOut> out(in.size());
  for (size_t i = 0; i < in.size(); i++) {
    CropOut& o = out[i];
    memset(&o, 0, sizeof(o));
    o.skip = crop_skips(in[i].c) ? 1u : 0u;
    const CropBounds b = crop_bounds(in[i].c, in[i].lo, in[i].hi, in[i].leaf);
    for (int a = 0; a < 3; a++) o.flo[a] = b.flo[a], o.fhi[a] = b.fhi[a];
    o.keep = crop_keeps(in[i].key, b) ? 1u : 0u;
  }
  f = fopen(argv[2], "wb");
  if (!f || (out.size() && fwrite(out.data(), sizeof(CropOut), out.size(), f) != out.size())) {
    fprintf(stderr, "cannot write %s\n", argv[2]);
    return 3;
  }
  fclose(f);
  return 0;
}
