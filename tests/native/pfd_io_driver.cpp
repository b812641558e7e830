// pfd_io_driver.cpp — host-only driver of the native .pfd reader (include/pfe_io.h) for the
// ASan + UBSan build in tests/test_pfd_native_sanitize.py.  Scans the files named on the command
// line with the given number of threads, fetches every field of every scanned file (and checks
// that a capacity one off is refused), packs each file alone and then every group of files that
// share shape and byte order, and prints one line per file:
//   <index> <status> <big_endian> <npart> <nsub> <proflen> <numdms> <rows> <stat_rows> <fnv64>
// the hash over the info's scalars, the fetched fields and the file's packed cube, subfreqs and
// scal -- so that the test can compare the sanitized reader's results with the product library's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pfe_io.h"

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* c = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
  return h;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <threads> <file>...\n", argv[0]);
    return 2;
  }
  const int threads = std::atoi(argv[1]);
  const int64_t n = argc - 2;
  pfe_pfd_batch* b = nullptr;
  if (pfe_pfd_scan(argv + 2, n, threads, &b) != 0 || !b) return 3;
  if (pfe_pfd_count(b) != n) return 4;
  std::vector<pfe_pfd_info> info((size_t)n);
  if (pfe_pfd_info_all(b, info.data(), n) != 0) return 5;
  if (n > 0 && pfe_pfd_info_all(b, info.data(), n - 1) == 0) return 6;  // too small a capacity
  for (int64_t i = 0; i < n; ++i) {
    const pfe_pfd_info& I = info[(size_t)i];
    uint64_t h = 1469598103934665603ull;
    if (I.status == PFE_IO_OK) {
      const int64_t nrec = (int64_t)I.npart * I.nsub, cube = nrec * I.proflen;
      h = fnv(h, I.scal, sizeof(I.scal));
      const int64_t counts[6] = {I.numdms, I.numperiods, I.numpdots, nrec * 7, I.nsub, PFE_PFD_NHEAD};
      for (int f = 0; f < 6; ++f) {
        std::vector<double> buf((size_t)counts[f]);  // exactly the field: an overrun is seen
        if (pfe_pfd_fetch(b, i, f, buf.data(), counts[f]) != 0) return 7;
        h = fnv(h, buf.data(), buf.size() * sizeof(double));
        if (pfe_pfd_fetch(b, i, f, buf.data(), counts[f] + 1) == 0) return 8;
        if (counts[f] > 0 && pfe_pfd_fetch(b, i, f, buf.data(), counts[f] - 1) == 0) return 8;
      }
      for (int f = 0; f < 6; ++f) {
        std::vector<char> buf((size_t)I.slen[f]);
        if (pfe_pfd_fetch(b, i, PFE_PFD_F_FILENM + f, buf.data(), I.slen[f]) != 0) return 9;
        h = fnv(h, buf.data(), buf.size());
      }
      if (pfe_pfd_fetch(b, i, 99, nullptr, 0) == 0) return 10;
      std::vector<uint64_t> words((size_t)cube);
      std::vector<double> sf((size_t)I.nsub), sc(8);
      if (pfe_pfd_pack(b, &i, 1, threads, words.data(), sf.data(), sc.data()) != 0) return 11;
      h = fnv(h, words.data(), words.size() * 8);
      h = fnv(h, sf.data(), sf.size() * 8);
      h = fnv(h, sc.data(), sc.size() * 8);
      if (pfe_pfd_pack(b, &i, 1, threads, nullptr, nullptr, nullptr) != 0) return 12;
    } else {
      double d;
      if (pfe_pfd_fetch(b, i, PFE_PFD_F_DMS, &d, 1) == 0) return 13;
      if (pfe_pfd_pack(b, &i, 1, threads, nullptr, nullptr, nullptr) == 0) return 14;
    }
    std::printf("%lld %d %d %d %d %d %d %lld %lld %016llx\n", (long long)i, I.status, I.big_endian,
                I.npart, I.nsub, I.proflen, I.numdms, (long long)I.rows, (long long)I.stat_rows,
                (unsigned long long)h);
  }
  // out-of-range rows are refused
  const int64_t bad[2] = {n, -1};
  if (pfe_pfd_pack(b, bad, 1, threads, nullptr, nullptr, nullptr) == 0 ||
      pfe_pfd_pack(b, bad + 1, 1, threads, nullptr, nullptr, nullptr) == 0)
    return 15;
  // every group of one shape and byte order, packed together by the thread pool
  std::vector<char> done((size_t)n, 0);
  for (int64_t i = 0; i < n; ++i) {
    const pfe_pfd_info& A = info[(size_t)i];
    if (done[(size_t)i] || A.status != PFE_IO_OK) continue;
    std::vector<int64_t> rows;
    for (int64_t j = i; j < n; ++j) {
      const pfe_pfd_info& B = info[(size_t)j];
      if (B.status == PFE_IO_OK && B.npart == A.npart && B.nsub == A.nsub &&
          B.proflen == A.proflen && B.big_endian == A.big_endian) {
        rows.push_back(j);
        done[(size_t)j] = 1;
      }
    }
    const size_t r = rows.size(), cube = (size_t)A.npart * A.nsub * A.proflen;
    std::vector<uint64_t> words(r * cube);
    std::vector<double> sf(r * A.nsub), sc(r * 8);
    if (pfe_pfd_pack(b, rows.data(), (int64_t)r, threads, words.data(), sf.data(), sc.data()) != 0)
      return 16;
    uint64_t h = fnv(1469598103934665603ull, words.data(), words.size() * 8);
    h = fnv(h, sf.data(), sf.size() * 8);
    h = fnv(h, sc.data(), sc.size() * 8);
    std::printf("pack %lld %zu %016llx\n", (long long)i, r, (unsigned long long)h);
    // a file of another group among them is refused
    for (int64_t j = 0; j < n; ++j) {
      if (info[(size_t)j].status == PFE_IO_OK && !done[(size_t)j]) {
        const int64_t mixed[2] = {i, j};
        if (pfe_pfd_pack(b, mixed, 2, threads, nullptr, nullptr, nullptr) == 0) return 17;
        break;
      }
    }
  }
  pfe_pfd_free(b);
  pfe_pfd_free(nullptr);
  return 0;
}
