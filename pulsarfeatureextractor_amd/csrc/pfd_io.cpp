// pfd_io.cpp — native PRESTO .pfd reader and cube packer of libpfe.so (host code; declared in
// include/pfe_io.h).  The header is parsed as pfd.read parses it (PFDFile.py:96-252); the cube
// never passes through this code's hands value by value: pfe_pfd_pack preads it from the file
// straight into the caller's slab, in the file's byte order, and the PFD calls deal with the
// byte order on the device (PFE_FLAG_PFD_BSWAP).  Only the header values, dms / periods / pdots
// and the foldstats (for the prof_var sum) are converted here.
//
// This file is built for a little-endian host (every ROCm host is): "big-endian" means
// byte-reversed.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pfe.h"
#include "../../include/pfe_io.h"

namespace {

constexpr int MAX_AUTO_THREADS = 16;    // nthreads <= 0 on a shared machine
constexpr double MAX_CUBE_BYTES = 1125899906842624.0;  // 2^50: int64 offsets cannot overflow

struct PfdFile {
  std::string path;
  pfe_pfd_info info{};
  std::vector<double> dms, periods, pdots;
  std::string str[6];
  double head[PFE_PFD_NHEAD] = {};
  double subdelta = 0.0, losub = 0.0;
};

struct Fd {
  int fd = -1;
  explicit Fd(const char* p) { fd = ::open(p, O_RDONLY | O_CLOEXEC); }
  ~Fd() {
    if (fd >= 0) ::close(fd);
  }
  Fd(const Fd&) = delete;
  Fd& operator=(const Fd&) = delete;
};

// exactly n bytes at off, or false (error or end of file)
bool pread_all(int fd, void* dst, size_t n, int64_t off) {
  char* d = static_cast<char*>(dst);
  while (n > 0) {
    const ssize_t r = ::pread(fd, d, n, (off_t)off);
    if (r < 0) {
      if (errno == EINTR) continue;
      return false;
    }
    if (r == 0) return false;
    d += r;
    off += r;
    n -= (size_t)r;
  }
  return true;
}

inline uint32_t load_u32(const uint8_t* p, bool be) {
  uint32_t v;
  std::memcpy(&v, p, 4);
  return be ? __builtin_bswap32(v) : v;
}
inline int32_t load_i32(const uint8_t* p, bool be) { return (int32_t)load_u32(p, be); }
inline double load_f64(const uint8_t* p, bool be) {
  uint64_t v;
  std::memcpy(&v, p, 8);
  if (be) v = __builtin_bswap64(v);
  double d;
  std::memcpy(&d, &v, 8);
  return d;
}

// the front of a file, read as the parser asks for it: take(n) is pfd.read's, false where
// that raises struct.error (the file ends first)
struct Front {
  int fd;
  int64_t size;
  std::vector<uint8_t> buf;
  int64_t pos = 0;
  bool io_error = false;
  Front(int fd_, int64_t size_) : fd(fd_), size(size_) {}
  const uint8_t* take(int64_t n) {
    if (n < 0 || pos + n > size) return nullptr;
    const int64_t need = pos + n;
    if (need > (int64_t)buf.size()) {
      const int64_t have = (int64_t)buf.size();
      const int64_t upto = std::min<int64_t>(size, std::max<int64_t>(need, have + 4096));
      buf.resize((size_t)upto);
      if (!pread_all(fd, buf.data() + have, (size_t)(upto - have), have)) {
        io_error = true;
        return nullptr;
      }
    }
    const uint8_t* p = buf.data() + pos;
    pos += n;
    return p;
  }
};

bool posn_chars(const uint8_t* p) {
  for (int i = 0; i < 16; ++i) {
    const uint8_t c = p[i];
    if (!((c >= '0' && c <= '9') || c == ':' || c == '.' || c == '-' || c == 0)) return false;
  }
  return true;
}
// test[: test.find(b"\0")]: up to the first NUL; without one, find gives -1: all but the last
std::string posn_string(const uint8_t* p) {
  const void* z = std::memchr(p, 0, 16);
  const size_t n = z ? (size_t)(static_cast<const uint8_t*>(z) - p) : 15;
  return std::string(reinterpret_cast<const char*>(p), n);
}

void scan_file(PfdFile& F) {
  pfe_pfd_info& I = F.info;
  I = pfe_pfd_info{};
  I.status = PFE_IO_ERR_OPEN;
  Fd f(F.path.c_str());
  if (f.fd < 0) return;
  struct stat sb;
  if (::fstat(f.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return;
  Front in(f.fd, (int64_t)sb.st_size);
  // a failed take: the file ends here (struct.error) unless the read itself failed
  auto cut = [&](int status) { I.status = in.io_error ? PFE_IO_ERR_OPEN : status; };

  const uint8_t* p = in.take(20);
  if (!p) return cut(PFE_IO_ERR_HEADER);
  bool be = false;
  for (int k = 0; k < 5; ++k)  // abs() of the int as a float64: INT_MIN has one
    if (std::fabs((double)load_i32(p + 4 * k, false)) > 100000.0) be = true;
  I.big_endian = be;
  I.numdms = load_i32(p, be);
  I.numperiods = load_i32(p + 4, be);
  I.numpdots = load_i32(p + 8, be);
  I.nsub = load_i32(p + 12, be);
  I.npart = load_i32(p + 16, be);
  if (!(p = in.take(28))) return cut(PFE_IO_ERR_HEADER);
  I.proflen = load_i32(p, be);
  I.numchan = load_i32(p + 4, be);
  for (int k = 0; k < 4; ++k) {
    if (!(p = in.take(4))) return cut(PFE_IO_ERR_HEADER);
    const int32_t ln = load_i32(p, be);
    if (ln < 0) {
      I.status = PFE_IO_ERR_VALUE;
      return;
    }
    if (!(p = in.take(ln))) return cut(PFE_IO_ERR_HEADER);
    F.str[k].assign(reinterpret_cast<const char*>(p), (size_t)ln);
  }
  if (!(p = in.take(16))) return cut(PFE_IO_ERR_HEADER);
  double* H = F.head;
  if (posn_chars(p)) {
    I.has_posn = 1;
    F.str[4] = posn_string(p);
    if (!(p = in.take(16))) return cut(PFE_IO_ERR_HEADER);
    F.str[5] = posn_string(p);
    if (!(p = in.take(16))) return cut(PFE_IO_ERR_HEADER);
  } else {
    F.str[4] = F.str[5] = "Unknown";
  }
  H[0] = load_f64(p, be);  // dt, startT
  H[1] = load_f64(p + 8, be);
  if (!(p = in.take(56))) return cut(PFE_IO_ERR_HEADER);
  for (int k = 0; k < 7; ++k) H[2 + k] = load_f64(p + 8 * k, be);  // endT .. bestdm
  for (int k = 0; k < 3; ++k) {  // topo, bary, fold: two floats, then p1, p2, p3
    if (!(p = in.take(8)) || !(p = in.take(24))) return cut(PFE_IO_ERR_HEADER);
    H[9 + k] = load_f64(p, be);
  }
  if (!(p = in.take(56))) return cut(PFE_IO_ERR_HEADER);
  for (int k = 0; k < 7; ++k) H[12 + k] = load_f64(p + 8 * k, be);  // orb
  // counts this reader does not take on go to pfd.read, whatever it makes of them
  if (I.numdms < 1 || I.numperiods < 0 || I.numpdots < 0 || I.nsub < 1 || I.npart < 1 ||
      I.proflen < 1 ||
      (double)I.npart * (double)I.nsub * (double)I.proflen * 8.0 > MAX_CUBE_BYTES) {
    I.status = PFE_IO_ERR_VALUE;
    return;
  }
  struct {
    std::vector<double>* v;
    int32_t n;
  } arrays[3] = {{&F.dms, I.numdms}, {&F.periods, I.numperiods}, {&F.pdots, I.numpdots}};
  for (auto& a : arrays) {
    if (!(p = in.take(8 * (int64_t)a.n))) return cut(PFE_IO_ERR_HEADER);
    a.v->resize((size_t)a.n);
    for (int32_t k = 0; k < a.n; ++k) (*a.v)[(size_t)k] = load_f64(p + 8 * (int64_t)k, be);
  }
  for (int k = 0; k < 6; ++k) I.slen[k] = (int32_t)F.str[k].size();

  // the cube: complete rows only; a little-endian file may end inside it (the rest reads as
  // zeros, and no foldstats follow), a big-endian one may not
  const int64_t nrows = (int64_t)I.npart * I.nsub, nprof = nrows * I.proflen;
  I.cube_off = in.pos;
  const int64_t avail = std::min<int64_t>(nprof, (in.size - in.pos) / 8);
  I.rows = avail / I.proflen;
  if (be && avail < nprof) {
    I.status = PFE_IO_ERR_CUBE;
    return;
  }
  I.stats_off = I.cube_off + nprof * 8;
  I.stat_rows = I.rows < nrows ? 0 : std::min<int64_t>(nrows, (in.size - I.stats_off) / 56);

  // varprof: prof_var (column 5) of every foldstats record, part-major then sub, added in that
  // order onto 0.0.  A record that is not there is zeros in pfd.read, and x + 0.0 = x for
  // every x such a sum can hold (it starts at +0.0, so it is never -0.0): the records present
  // give the same bits.
  double varprof = 0.0;
  if (I.stat_rows > 0) {
    constexpr int64_t BLOCK = 4096;  // records per read
    std::vector<uint8_t> sbuf((size_t)(std::min(BLOCK, I.stat_rows) * 56));
    for (int64_t r0 = 0; r0 < I.stat_rows; r0 += BLOCK) {
      const int64_t rn = std::min(BLOCK, I.stat_rows - r0);
      if (!pread_all(f.fd, sbuf.data(), (size_t)(rn * 56), I.stats_off + r0 * 56)) {
        I.status = PFE_IO_ERR_OPEN;
        return;
      }
      for (int64_t r = 0; r < rn; ++r) varprof += load_f64(sbuf.data() + r * 56 + 40, be);
    }
  }

  // the derived quantities (PFDFile.py:219-252), each operation rounded on its own
  const double fold_p1 = H[11], lofreq = H[6], chan_wid = H[7];
  // (the products through a volatile: no compiler setting may contract them into an fma)
  const double binspersec = fold_p1 * (double)I.proflen;
  int64_t cps = (int64_t)I.numchan / I.nsub;  // Python's floor division
  if ((int64_t)I.numchan % I.nsub != 0 && I.numchan < 0) --cps;
  I.chanpersub = (int32_t)cps;
  volatile double prod = chan_wid * (double)cps;
  const double subdelta = prod;
  const double losub = lofreq + subdelta - chan_wid;
  F.subdelta = subdelta;
  F.losub = losub;
  H[19] = binspersec;
  H[20] = subdelta;
  H[21] = losub;
  H[22] = varprof;
  I.scal[PFE_PFD_BESTDM] = H[8];
  I.scal[PFE_PFD_BINSPERSEC] = binspersec;
  I.scal[PFE_PFD_AVGPROF] = std::numeric_limits<double>::quiet_NaN();
  I.scal[PFE_PFD_VARPROF] = varprof;
  I.scal[PFE_PFD_DM_LO] = F.dms.front();
  I.scal[PFE_PFD_DM_HI] = F.dms.back();
  I.scal[PFE_PFD_NUMDMS] = (double)I.numdms;
  I.scal[PFE_PFD_BARY_P1] = H[10];
  I.status = PFE_IO_OK;
}

// numpy's arange(nsub, dtype="d") * subdeltafreq + losubfreq: a product and a sum, each rounded
void fill_subfreqs(const PfdFile& F, double* dst) {
  for (int32_t k = 0; k < F.info.nsub; ++k) {
    volatile double prod = (double)k * F.subdelta;  // no contraction into an fma
    dst[k] = prod + F.losub;
  }
}

template <class Fn>
void parallel_for(int64_t n, int nthreads, Fn&& fn) {
  if (nthreads <= 0)
    nthreads = (int)std::min<unsigned>(MAX_AUTO_THREADS,
                                       std::max(1u, std::thread::hardware_concurrency()));
  nthreads = (int)std::min<int64_t>(nthreads, std::max<int64_t>(1, n));
  std::atomic<int64_t> next{0};
  auto work = [&] {
    for (int64_t i; (i = next.fetch_add(1)) < n;) fn(i);
  };
  if (nthreads == 1) {
    work();
    return;
  }
  std::vector<std::thread> th;
  th.reserve((size_t)nthreads);
  for (int t = 0; t < nthreads; ++t) th.emplace_back(work);
  for (auto& t : th) t.join();
}

}  // namespace

struct pfe_pfd_batch {
  std::vector<PfdFile> files;
};

extern "C" {

int pfe_pfd_scan(const char* const* paths, int64_t n, int32_t nthreads, pfe_pfd_batch** out) {
  if (!out || n < 0 || (n > 0 && !paths)) return PFE_EINVAL;
  for (int64_t i = 0; i < n; ++i)
    if (!paths[i]) return PFE_EINVAL;
  pfe_pfd_batch* b = new pfe_pfd_batch;
  b->files.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) b->files[(size_t)i].path = paths[i];
  parallel_for(n, nthreads, [&](int64_t i) { scan_file(b->files[(size_t)i]); });
  *out = b;
  return PFE_OK;
}

int64_t pfe_pfd_count(const pfe_pfd_batch* b) { return b ? (int64_t)b->files.size() : 0; }

int pfe_pfd_info_all(const pfe_pfd_batch* b, pfe_pfd_info* out, int64_t capacity) {
  if (!b || capacity < (int64_t)b->files.size() || (!out && !b->files.empty())) return PFE_EINVAL;
  for (size_t i = 0; i < b->files.size(); ++i) out[i] = b->files[i].info;
  return PFE_OK;
}

int pfe_pfd_fetch(const pfe_pfd_batch* b, int64_t i, int32_t field, void* dst, int64_t capacity) {
  if (!b || i < 0 || i >= (int64_t)b->files.size() || (!dst && capacity != 0)) return PFE_EINVAL;
  const PfdFile& F = b->files[(size_t)i];
  const pfe_pfd_info& I = F.info;
  if (I.status != PFE_IO_OK) return PFE_EINVAL;
  auto doubles = [&](const double* src, int64_t count) {
    if (capacity != count) return (int)PFE_EINVAL;
    if (count) std::memcpy(dst, src, (size_t)count * sizeof(double));
    return (int)PFE_OK;
  };
  switch (field) {
    case PFE_PFD_F_DMS: return doubles(F.dms.data(), (int64_t)F.dms.size());
    case PFE_PFD_F_PERIODS: return doubles(F.periods.data(), (int64_t)F.periods.size());
    case PFE_PFD_F_PDOTS: return doubles(F.pdots.data(), (int64_t)F.pdots.size());
    case PFE_PFD_F_HEAD: return doubles(F.head, PFE_PFD_NHEAD);
    case PFE_PFD_F_SUBFREQS:
      if (capacity != I.nsub) return PFE_EINVAL;
      fill_subfreqs(F, static_cast<double*>(dst));
      return PFE_OK;
    case PFE_PFD_F_STATS: {
      const int64_t nrec = (int64_t)I.npart * I.nsub;
      if (capacity != nrec * 7) return PFE_EINVAL;
      double* d = static_cast<double*>(dst);
      std::memset(d, 0, (size_t)(nrec * 56));
      if (I.stat_rows == 0) return PFE_OK;
      Fd f(F.path.c_str());
      if (f.fd < 0 || !pread_all(f.fd, d, (size_t)(I.stat_rows * 56), I.stats_off)) return PFE_EINVAL;
      if (I.big_endian) {
        for (int64_t k = 0; k < I.stat_rows * 7; ++k)
          d[k] = load_f64(reinterpret_cast<const uint8_t*>(d + k), true);
      }
      return PFE_OK;
    }
    default: break;
  }
  if (field >= PFE_PFD_F_FILENM && field <= PFE_PFD_F_DECSTR) {
    const std::string& s = F.str[field - PFE_PFD_F_FILENM];
    if (capacity != (int64_t)s.size()) return PFE_EINVAL;
    if (!s.empty()) std::memcpy(dst, s.data(), s.size());
    return PFE_OK;
  }
  return PFE_EINVAL;
}

int pfe_pfd_pack(const pfe_pfd_batch* b, const int64_t* rows, int64_t nrows, int32_t nthreads,
                 void* profs_raw, double* subfreqs, double* scal) {
  if (!b || nrows < 0 || (nrows > 0 && !rows)) return PFE_EINVAL;
  if (nrows == 0) return PFE_OK;
  const int64_t nf = (int64_t)b->files.size();
  for (int64_t r = 0; r < nrows; ++r)
    if (rows[r] < 0 || rows[r] >= nf || b->files[(size_t)rows[r]].info.status != PFE_IO_OK)
      return PFE_EINVAL;
  const pfe_pfd_info& first = b->files[(size_t)rows[0]].info;
  for (int64_t r = 1; r < nrows; ++r) {
    const pfe_pfd_info& I = b->files[(size_t)rows[r]].info;
    if (I.npart != first.npart || I.nsub != first.nsub || I.proflen != first.proflen ||
        I.big_endian != first.big_endian)
      return PFE_EINVAL;
  }
  const int64_t cube = (int64_t)first.npart * first.nsub * first.proflen * 8;
  std::atomic<int> bad{0};
  parallel_for(nrows, nthreads, [&](int64_t r) {
    const PfdFile& F = b->files[(size_t)rows[r]];
    const pfe_pfd_info& I = F.info;
    if (profs_raw) {
      char* dst = static_cast<char*>(profs_raw) + r * cube;
      const int64_t got = I.rows * I.proflen * 8;  // complete rows; the rest reads as zeros
      Fd f(F.path.c_str());
      if (f.fd < 0 || (got > 0 && !pread_all(f.fd, dst, (size_t)got, I.cube_off))) {
        bad.store(1);
        return;
      }
      if (got < cube) std::memset(dst + got, 0, (size_t)(cube - got));
    }
    if (subfreqs) fill_subfreqs(F, subfreqs + r * I.nsub);
    if (scal) std::memcpy(scal + r * PFE_PFD_NSCAL, I.scal, sizeof(I.scal));
  });
  return bad.load() ? PFE_EINVAL : PFE_OK;
}

void pfe_pfd_free(pfe_pfd_batch* b) { delete b; }

}  // extern "C"
