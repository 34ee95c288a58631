// Host build of the device decoder's inflate core (revo_amd/csrc/revo_inflate.h), one lane.
//   inflate_harness <records in> <results out>
// records: [u64 compressed length][u64 expected output length][compressed bytes] ...
// results: [i32 status (rinf::OK or an rinf::E_* code)][expected-length output bytes] per record.
// Every buffer is allocated at its exact size, so a sanitizer build catches any read or write out of range.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../revo_amd/csrc/revo_inflate.h"

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <records> <results>\n", argv[0]); return 2; }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) { perror("open"); return 2; }
  std::vector<uint8_t> ring(rinf::RING), win(rinf::IN_WIN), lens(rinf::MAX_LENS);
  std::vector<uint16_t> t(2 * (16 + 16 + rinf::FAST) + rinf::MAX_LIT + rinf::MAX_DIST);
  uint16_t* q = t.data();
  rinf::Mem m;
  m.ring = ring.data(); m.win = win.data(); m.lens = lens.data();
  m.lcount = q; q += 16; m.loffs = q; q += 16; m.lsym = q; q += rinf::MAX_LIT; m.lfast = q; q += rinf::FAST;
  m.dcount = q; q += 16; m.doffs = q; q += 16; m.dsym = q; q += rinf::MAX_DIST; m.dfast = q;
  uint64_t hdr[2];
  while (fread(hdr, sizeof(hdr), 1, fi) == 1) {
    uint8_t* in = (uint8_t*)malloc(hdr[0] ? hdr[0] : 1);
    uint8_t* out = (uint8_t*)malloc(hdr[1] ? hdr[1] : 1);
    if (!in || !out || (hdr[0] && fread(in, hdr[0], 1, fi) != 1)) { fprintf(stderr, "bad record\n"); return 2; }
    memset(out, 0, hdr[1] ? hdr[1] : 1);
    rinf::Inflater<rinf::HostPar> inf(rinf::HostPar(), m, in, hdr[0], out, hdr[1]);
    const int32_t st = inf.run();
    fwrite(&st, sizeof(st), 1, fo);
    if (hdr[1]) fwrite(out, hdr[1], 1, fo);
    free(in);
    free(out);
  }
  fclose(fi);
  fclose(fo);
  return 0;
}
