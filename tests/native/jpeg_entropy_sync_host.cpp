// Host driver of ops/csrc/jpeg_entropy_sync.h, the lane run jpeg_entropy_sync_kernel runs per chunk
// (tests/test_jpeg_entropy_sync_native.py builds it plain and with ASan + UBSan on the host).
//
//   jpeg_entropy_sync_host <cases.bin> <out.bin> <chunk_bytes>
//
// cases.bin: the format of jpeg_entropy_host.cpp ("JED1", uint32 count, then per case uint32 nb,
// mcus, per, nint, nbytes, mutate; uint32 tables[JPEG_DEC_WORDS]; uint32 intervals[nint][2];
// nbytes bytes).  out.bin: per case uint32 flag, rounds, chunks, int16 coef[mcus * nb * 64] of
// the chunked decode (whatever it left when flagged).
//
// The chunked entropy decode contract, serially over the lanes: Jacobi rounds, valid chain, block
// scan, write pass, DC pass, check pass.  Every interval is decoded from a heap copy of exactly
// its length and into a coefficient buffer of exactly the case's size, so a read or a store one
// element outside either is a sanitizer report.  Then the mutation pass: for every case marked
// `mutate`, single-bit flips and truncations chosen by a fixed-seed generator (at most 2000 runs
// in all, 16-byte chunks); each run is decoded chunked and by jpeg_decode_interval, and has to
// keep the contract's two implications: serial OK => no flag and equal coefficients, serial
// error => flag.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_entropy_sync.h"

namespace {

struct Case {
  uint32_t nb, mcus, per, nint, nbytes, mutate;
  std::vector<uint32_t> tables, intervals;
  std::vector<uint8_t> bytes;
};

struct Result {
  bool flag = false;
  uint32_t rounds = 0, chunks = 0;
};

bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

uint32_t chunk_bytes_for(const Case& c, const std::vector<uint32_t>& ivals, uint32_t want) {
  uint32_t longest = 0;
  for (uint32_t it = 0; it < c.nint; ++it) longest = ivals[2 * it + 1] > longest ? ivals[2 * it + 1] : longest;
  const uint32_t need = (longest + JPEG_SYNC_MAX_CHUNKS - 1) / JPEG_SYNC_MAX_CHUNKS;
  uint32_t cb = want > need ? want : need;
  if (cb < 16) cb = 16;
  return (cb + 15) / 16 * 16;
}

Result decode_chunked(const Case& c, const std::vector<uint8_t>& bytes, const std::vector<uint32_t>& ivals,
                      uint32_t want, int16_t* coef) {
  Result res;
  const uint32_t cb = chunk_bytes_for(c, ivals, want);
  const uint32_t* tabs = c.tables.data();
  const int nb = (int)c.nb;
  uint64_t completed = 0;
  for (uint32_t it = 0; it < c.nint; ++it) {
    const uint32_t off = ivals[2 * it], len = ivals[2 * it + 1];
    const uint64_t m0 = (uint64_t)it * c.per;
    if (m0 >= c.mcus || off > bytes.size() || len > bytes.size() - off || len >= JPEG_SYNC_MAX_LEN) {
      res.flag = true;
      continue;
    }
    const uint32_t left = c.mcus - (uint32_t)m0;
    const int nblk = (int)(left < c.per ? left : c.per) * nb;
    int16_t* out = coef + (size_t)m0 * c.nb * 64;
    const uint32_t n = (len + cb - 1) / cb;
    res.chunks += n;
    if (n == 0) continue;
    uint8_t* own = static_cast<uint8_t*>(malloc(len));                  // exactly the interval
    memcpy(own, bytes.data() + off, len);
    std::vector<uint32_t> start(n), exits(n, JPEG_SYNC_ERR), blocks(n, 0);
    std::vector<uint8_t> run(n, 1), next(n, 0);
    auto begin = [cb](uint32_t l) { return l * cb; };
    auto end = [cb, len](uint32_t l) { return (l + 1) * cb < len ? (l + 1) * cb : len; };
    start[0] = 0;
    for (uint32_t l = 1; l < n; ++l) start[l] = jpeg_sync_pack(jpeg_sync_guess(own, len, begin(l)), 0, 0, begin(l));
    bool any = true;
    uint32_t rounds = 0;
    for (uint32_t r = 0; r < n && any; ++r) {
      ++rounds;
      for (uint32_t l = 0; l < n; ++l) {
        if (!run[l]) continue;
        JpegSyncRun s;
        jpeg_sync_unpack(start[l], begin(l), s);
        jpeg_sync_lane_run<false>(own, len, end(l), tabs, nb, s, 0, 0, nullptr);
        blocks[l] = s.blocks;
        exits[l] = s.err != JPEG_DEC_OK ? JPEG_SYNC_ERR : jpeg_sync_pack(s.p, s.blk, s.k, end(l));
      }
      any = false;
      for (uint32_t l = 1; l < n; ++l) {
        next[l] = exits[l - 1] != JPEG_SYNC_ERR && exits[l - 1] != start[l];
        if (next[l]) {
          start[l] = exits[l - 1];
          any = true;
        }
      }
      run.swap(next);
      run[0] = 0;
    }
    if (rounds > res.rounds) res.rounds = rounds;
    long long first = 0;
    for (uint32_t l = 0; l < n; ++l) {                                   // the valid chain, in order
      if (l > 0 && exits[l - 1] == JPEG_SYNC_ERR) break;
      JpegSyncRun s;
      jpeg_sync_unpack(start[l], begin(l), s);
      const long long at = first - (s.k != 0 ? 1 : 0);
      if (at < nblk) {
        jpeg_sync_lane_run<true>(own, len, end(l), tabs, nb, s, (int)at, nblk, out);
        if (s.err != JPEG_DEC_OK && s.err_block < nblk) res.flag = true;
        completed += s.done;
      }
      first += blocks[l];
    }
    free(own);
    for (int comp = 0; comp < 3; ++comp) {                               // DC pass
      uint32_t pred = 0;
      const uint32_t q0 = tabs[comp == 0 ? 0 : 64];
      for (int g = 0; g < nblk; ++g) {
        const int blk = g % nb;
        if (comp == 0 ? blk >= nb - 2 : blk != nb - 3 + comp) continue;
        pred += (uint32_t)(int)out[(size_t)g * 64];
        const bool ok = jpeg_sync_dc_ok(pred, q0);
        out[(size_t)g * 64] = ok ? (int16_t)(int32_t)pred : (int16_t)0;
        if (!ok) res.flag = true;
      }
    }
  }
  for (size_t g = 0; g < (size_t)c.mcus * c.nb; ++g)                     // check pass
    if (!jpeg_sync_block_ok(coef + g * 64, tabs + ((int)(g % c.nb) < nb - 2 ? 0 : 64))) res.flag = true;
  if (completed != (uint64_t)c.mcus * c.nb) res.flag = true;
  return res;
}

// the serial decoder on the same bytes: the status of the lowest failing interval
int decode_serial(const Case& c, const std::vector<uint8_t>& bytes, const std::vector<uint32_t>& ivals, int16_t* coef) {
  int first = JPEG_DEC_OK;
  for (uint32_t it = 0; it < c.nint; ++it) {
    const uint32_t off = ivals[2 * it], len = ivals[2 * it + 1];
    int st;
    const uint64_t m0 = (uint64_t)it * c.per;
    if (m0 >= c.mcus) {
      st = JPEG_DEC_OVERRUN;
    } else if (off > bytes.size() || len > bytes.size() - off) {
      st = JPEG_DEC_TRUNCATED;
    } else {
      uint8_t* own = static_cast<uint8_t*>(malloc(len ? len : 1));
      if (len) memcpy(own, bytes.data() + off, len);
      const uint32_t left = c.mcus - (uint32_t)m0;
      st = jpeg_decode_interval(own, len, c.tables.data(), (int)c.nb, (int)(left < c.per ? left : c.per),
                                coef + (size_t)m0 * c.nb * 64);
      free(own);
    }
    if (st != JPEG_DEC_OK && first == JPEG_DEC_OK) first = st;
  }
  return first;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s cases.bin out.bin chunk_bytes\n", argv[0]);
    return 2;
  }
  const uint32_t want = (uint32_t)atoi(argv[3]);
  if (want < 16 || want > (1u << 20)) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  char magic[4];
  uint32_t count = 0;
  if (!rd(f, magic, 4) || memcmp(magic, "JED1", 4) != 0 || !rd(f, &count, 4)) return 2;
  std::vector<Case> cases(count);
  for (Case& c : cases) {
    uint32_t h[6];
    if (!rd(f, h, sizeof h)) return 2;
    c.nb = h[0]; c.mcus = h[1]; c.per = h[2]; c.nint = h[3]; c.nbytes = h[4]; c.mutate = h[5];
    if ((c.nb != 3 && c.nb != 6) || c.per == 0 || c.mcus == 0 || c.mcus > (1u << 20) || c.nint > (1u << 20)) return 2;
    c.tables.resize(JPEG_DEC_WORDS);
    c.intervals.resize(2 * (size_t)c.nint);
    c.bytes.resize(c.nbytes);
    if (!rd(f, c.tables.data(), 4 * c.tables.size()) || !rd(f, c.intervals.data(), 4 * c.intervals.size()) ||
        !rd(f, c.bytes.data(), c.nbytes))
      return 2;
  }
  fclose(f);

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (const Case& c : cases) {
    const size_t n = (size_t)c.mcus * c.nb * 64;
    int16_t* coef = static_cast<int16_t*>(calloc(n, sizeof(int16_t)));
    const Result r = decode_chunked(c, c.bytes, c.intervals, want, coef);
    const uint32_t head[3] = {r.flag ? 1u : 0u, r.rounds, r.chunks};
    fwrite(head, 4, 3, o);
    fwrite(coef, sizeof(int16_t), n, o);
    free(coef);
  }
  fclose(o);

  // mutation pass
  uint64_t seed = 0x9E3779B97F4A7C15ull;
  auto next = [&seed]() {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(seed >> 33);
  };
  size_t targets = 0;
  for (const Case& c : cases) targets += c.mutate && c.nbytes > 0;
  const int per_case = targets ? (int)(2000 / targets) : 0;
  long runs = 0, ok = 0, flagged = 0;
  for (const Case& c : cases) {
    if (!c.mutate || c.nbytes == 0) continue;
    const size_t n = (size_t)c.mcus * c.nb * 64;
    for (int k = 0; k < per_case; ++k) {
      std::vector<uint8_t> bytes = c.bytes;
      std::vector<uint32_t> ivals = c.intervals;
      if (k % 4 == 3) {                        // truncation of one interval
        const uint32_t it = next() % c.nint;
        if (ivals[2 * it + 1] > 0) ivals[2 * it + 1] = next() % ivals[2 * it + 1];
      } else {                                 // one flipped bit
        bytes[next() % c.nbytes] ^= (uint8_t)(1u << (next() & 7));
      }
      int16_t* a = static_cast<int16_t*>(calloc(n, sizeof(int16_t)));
      int16_t* b = static_cast<int16_t*>(calloc(n, sizeof(int16_t)));
      const Result r = decode_chunked(c, bytes, ivals, 16, a);
      const int st = decode_serial(c, bytes, ivals, b);
      const bool same = memcmp(a, b, n * sizeof(int16_t)) == 0;
      free(a);
      free(b);
      if (st == JPEG_DEC_OK ? (r.flag || !same) : !r.flag) {
        printf("mutation %ld: serial status %d, flag %d, coefficients %s\n", runs, st, (int)r.flag,
               same ? "equal" : "differ");
        return 1;
      }
      ok += st == JPEG_DEC_OK;
      flagged += r.flag;
      ++runs;
    }
  }
  printf("cases %u mutations %ld ok %ld flagged %ld\n", count, runs, ok, flagged);
  return 0;
}
