// Host driver for ops/csrc/jpeg_layout.h (tests/test_jpeg_layout_native.py): reads argument
// tuples, one per line, and prints every field of the layout they give, or the refusal.
//   E B H W s420 restart blocks optimized lj header_bytes   -> jpeg_encode_layout
//   D B H W s420 restart chunked nbytes ngroups              -> jpeg_decode_layout
#include <stdio.h>

#include "jpeg_layout.h"

static void print_geometry(const JpegGeometry& g) {
  printf("ok nb=%d mx=%d my=%d mcus=%lld restart=%lld per=%lld nint=%lld", g.nb, g.mx, g.my, g.mcus, g.restart, g.per, g.nint);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (f == nullptr) return 2;
  char kind;
  long long v[9];
  int lines = 0;
  while (fscanf(f, " %c", &kind) == 1) {
    const int want = kind == 'E' ? 9 : 8;
    for (int i = 0; i < want; ++i)
      if (fscanf(f, "%lld", &v[i]) != 1) return 3;
    if (kind == 'E') {
      const JpegEncodeLayout l = jpeg_encode_layout(v[0], v[1], v[2], v[3] != 0, v[4], v[5] != 0, v[6] != 0, v[7] != 0, v[8]);
      if (l.refusal != nullptr) {
        printf("refused %s\n", l.refusal);
      } else {
        print_geometry(l.g);
        printf(" coef=%lld work=%lld blk=%lld scratch=%lld hopt=%lld hdrs=%lld stride=%lld hdr_cap=%lld prefix=%lld err=%lld"
               " hdr_lens=%lld lens=%lld offs=%lld slack=%lld\n", l.coef, l.work, l.blk, l.scratch, l.hopt, l.hdrs, l.stride,
               l.hdr_cap, l.prefix, l.err, l.hdr_lens, l.lens, l.offs, l.slack);
      }
    } else if (kind == 'D') {
      const JpegDecodeLayout l = jpeg_decode_layout(v[0], v[1], v[2], v[3] != 0, v[4], v[5] != 0);
      if (l.refusal != nullptr) {
        printf("refused %s\n", l.refusal);
      } else {
        print_geometry(l.g);
        printf(" nivals=%lld ncoef=%lld buf=%lld planes=%lld staged_min=%lld sync_bytes=%lld\n", l.nivals, l.ncoef, l.buf,
               l.planes, l.staged_min(v[6]), l.sync_bytes(v[7]));
      }
    } else {
      return 3;
    }
    ++lines;
  }
  fclose(f);
  fprintf(stderr, "lines %d\n", lines);
  return 0;
}
