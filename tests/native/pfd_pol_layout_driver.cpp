// pfd_pol_layout_driver.cpp — stand-alone check of the scratch of the pfe_pfd_*_i16_pol calls
// (csrc/launch.h: pfd_f32_chunk and the int16 forms of pfd_dmprof_layout, pfd_scores_layout,
// pfd_avgprof_layout and pfd_scrunch_layout with a polarisation count) on a CPU, built with
// ASan + UBSan by tests/test_pfd_pol_layout_host.py.
//
// Each line of the case file (argv[1]) is one of
//   dmprof n npart nsub L host opt wts profile chis lyon8 ws_bytes avgprof npol nsum
//   scores n npart nsub L host opt wts groups k g_bytes cus tail avgprof npol nsum
//   avgprof n npart nsub L host 0 wts npol nsum
//   scrunch n npart nchan nbin host 0 wts rot fscr bscr npol nsum
// opt: PFE_OPT_PFD_F32_CHUNK; wts: weights are given; tail = 1: the layout of the shorter last
// pass (n % chunk folds); avgprof: PFE_FLAG_PFD_AVGPROF; npol, nsum: the polarisations stored
// and summed -- a host-pointer call stages the nsum that are read, compacted, so the layouts
// take nsum and never see npol.  The driver sizes the pass
// (pfd_f32_chunk), measures the layout (Arena{}), allocates exactly that many bytes, places
// (Arena{block}), fills every region over its whole length with a byte value of its own and reads
// all of them back (ASan sees an overrun, the read-back an overlap), checks each pointer of the
// returned struct against the region it is named for, writes the staged arrays and the part sums
// at the last element the kernels index (through the PfdI16Src a host-pointer call builds on
// them), and prints the chunk, `name bytes` per region and the total.  For a last pass it also
// checks that the staged arrays and the part sums lie where the full pass has them.  A failed
// check exits with status 2.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "launch.h"

using pfe::Arena;
using Trace = std::vector<Arena::Region>;

[[noreturn]] static void fail(const char* what, const char* name) {
  printf("FAIL %s %s\n", what, name);
  exit(2);
}

static const Arena::Region* find(const Trace& t, const char* name) {
  for (const Arena::Region& r : t)
    if (!strcmp(r.name, name)) return &r;
  return nullptr;
}

static void is(uintptr_t base, const Trace& t, const void* p, const char* name, bool taken) {
  const Arena::Region* r = find(t, name);
  if (!taken) {
    if (p || r) fail("region not asked for", name);
    return;
  }
  if (!r || p != (const void*)(base + r->off)) fail("pointer is not region", name);
}

struct Placed {
  unsigned char* block = nullptr;
  size_t total = 0;
  Trace t;
};

// measure, allocate exactly that, place, fill, read back
template <class Walk, class Check>
static void run(const std::string& line, Walk walk, Check check) {
  Trace tm;
  Arena m;
  m.trace = &tm;
  walk(m);
  Placed P;
  P.total = m.bytes();
  P.block = P.total ? (unsigned char*)aligned_alloc(256, P.total) : nullptr;
  if (P.total && !P.block) fail("aligned_alloc", line.c_str());
  Arena pl{(uintptr_t)P.block};
  pl.trace = &P.t;
  const auto s = walk(pl);
  if (pl.bytes() != P.total || P.t.size() != tm.size()) fail("measure and place disagree", line.c_str());
  for (size_t i = 0; i < P.t.size(); ++i) {
    const Arena::Region &a = P.t[i], &b = tm[i];
    if (a.off != b.off || a.bytes != b.bytes || strcmp(a.name, b.name))
      fail("measure and place disagree", a.name);
    if (a.off % 256 || a.off + a.bytes > P.total) fail("region out of the block", a.name);
  }
  for (size_t i = 0; i < P.t.size(); ++i)
    if (P.t[i].bytes) memset(P.block + P.t[i].off, (int)(i % 251 + 1), P.t[i].bytes);
  for (size_t i = 0; i < P.t.size(); ++i) {  // every byte still the region's own
    const unsigned char* r = P.block + P.t[i].off;
    if (P.t[i].bytes && (r[0] != (unsigned char)(i % 251 + 1) || memcmp(r, r + 1, P.t[i].bytes - 1)))
      fail("regions overlap", P.t[i].name);
  }
  if (P.block) check(P, s);
  for (const Arena::Region& r : P.t) printf("%s %zu\n", r.name, r.bytes);
  printf("total %zu\n", P.total);
  free(P.block);
}

// the four staged arrays as the kernels reach them: the dense strides of a cube of npol = nsum
// polarisations (what a host-pointer call stages) on the staged pointers, written at the last
// value of the last polarisation of the last fold; the weights through strides of their own
static int g_nsum = 1;
static void touch_staged(int16_t* data, float* scl, float* offs, float* wts, const pfe_pfd_in& v) {
  pfe_pfd_i16_in f{};
  f.data = data, f.scl = scl, f.offs = offs, f.wts = wts;
  f.npart = v.npart, f.nsub = v.nsub, f.proflen = v.proflen, f.n = v.n;
  const pfe::PfdI16Src q = pfe::pfd_i16_src(f, false, g_nsum, g_nsum).from(v.n - 1);
  if (q.nsum != g_nsum || pfe::pfd_i16_ns(q) != (g_nsum == 2 ? 2 : 0)) fail("kernels", "nsum");
  const int64_t p = v.npart - 1, k = g_nsum - 1, s = v.nsub - 1, b = v.proflen - 1;
  char* d = const_cast<char*>(q.data) + p * q.dps + k * q.dks + 2 * (s * (int64_t)v.proflen + b);
  if (d != (char*)(data + (size_t)v.n * v.npart * g_nsum * v.nsub * v.proflen - 1))
    fail("dense strides", "data16");
  *reinterpret_cast<int16_t*>(d) = 1;
  for (const char* a : {q.scl, q.offs})
    *reinterpret_cast<float*>(const_cast<char*>(a) + p * q.pps + k * q.pks + 4 * s) = 1.0f;
  if (const_cast<char*>(q.scl) + p * q.pps + k * q.pks + 4 * s !=
      (char*)(scl + (size_t)v.n * v.npart * g_nsum * v.nsub - 1))
    fail("dense strides", "scl16");
  if (q.wts) {
    char* w = const_cast<char*>(q.wts) + p * q.wps + 4 * s;
    if (w != (char*)(wts + (size_t)v.n * v.npart * v.nsub - 1)) fail("dense strides", "wts16");
    *reinterpret_cast<float*>(w) = 1.0f;
  }
}

// the staged arrays and the part sums: the pointers, and the last element each kernel touches
static void check_inputs(const Placed& P, const pfe::PfdInputs& in, const pfe_pfd_in& v, bool host,
                         bool wts, int64_t chunk) {
  const uintptr_t b = (uintptr_t)P.block;
  is(b, P.t, in.profs, "profs", false);  // an int16 call never stages doubles or floats
  is(b, P.t, in.profs32, "profs32", false);
  is(b, P.t, in.data16, "data16", host);
  is(b, P.t, in.scl16, "scl16", host);
  is(b, P.t, in.offs16, "offs16", host);
  is(b, P.t, in.wts16, "wts16", host && wts);
  is(b, P.t, in.subfreqs, "subfreqs", host);
  is(b, P.t, in.scal, "scal", host);
  is(b, P.t, in.psum, "psum", true);
  const size_t E = (size_t)v.nsub * v.proflen;
  if (host) touch_staged(in.data16, in.scl16, in.offs16, in.wts16, v);
  in.psum[(size_t)chunk * E - 1] = 1.0;
  if ((uintptr_t)in.psum % 256) fail("psum not 256-byte aligned", "psum");
}

static void check_avg(const Placed& P, const pfe::PfdAvgWork& w, const pfe_pfd_in& v, bool host,
                      bool avg, int64_t chunk) {
  const uintptr_t b = (uintptr_t)P.block;
  is(b, P.t, w.csum, "avg_csum", avg);
  is(b, P.t, w.scal, "avg_scal", avg && !host);
  if (!avg) return;
  const int64_t E = (int64_t)v.npart * v.nsub * v.proflen;
  w.csum[(size_t)chunk * pfe::pfd_avg_chunks(E) - 1] = 1.0;
  if (!host) w.scal[(size_t)v.n * PFE_PFD_NSCAL - 1] = 1.0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 64;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 65;
  char buf[256];
  while (fgets(buf, sizeof(buf), f)) {
    std::string line(buf);
    while (!line.empty() && (line.back() == '\n' || line.back() == ' ')) line.pop_back();
    if (line.empty()) continue;
    char kind[16];
    long long v[15] = {};
    const int got = sscanf(buf, "%15s %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld",
                           kind, v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9,
                           v + 10, v + 11, v + 12, v + 13, v + 14);
    const std::string k(kind);
    pfe_pfd_in in{};
    in.n = v[0], in.npart = (int)v[1], in.nsub = (int)v[2], in.proflen = (int)v[3];
    const bool host = v[4], wts = v[6];
    const int ki = wts ? pfe::PFD_I16_WEIGHTS : pfe::PFD_I16_PLAIN;
    const int64_t chunk = pfe::pfd_f32_chunk(in.nsub, in.proflen, in.n, v[5]);
    if (chunk < 1 || chunk > in.n) fail("chunk", line.c_str());
    if ((size_t)chunk * in.nsub * in.proflen * sizeof(double) > pfe::PFD_F32_PSUM_BUDGET && chunk != 1)
      fail("part sums beyond the budget", line.c_str());
    printf("case %s\nchunk %lld\n", line.c_str(), (long long)chunk);
    // npol, nsum: the last two numbers of every line
    const int npol = (int)v[got - 3], nsum = (int)v[got - 2];
    if (got < 10 || npol < 1 || npol > 4 || nsum < 1 || nsum > 2 || nsum > npol) fail("npol, nsum", line.c_str());
    g_nsum = nsum;
    if (k == "dmprof" && got == 15) {
      const bool avg = v[11];
      run(line,
          [&](Arena& A) {
            return pfe::pfd_dmprof_layout(A, in, host, v[7], v[8], v[9], (size_t)v[10], chunk, avg,
                                          false, ki, 0, nsum);
          },
          [&](const Placed& P, const pfe::PfdDmprofStage& s) {
            const uintptr_t b = (uintptr_t)P.block;
            check_inputs(P, s.in, in, host, wts, chunk);
            check_avg(P, s.avg, in, host, avg, chunk);
            is(b, P.t, s.profile, "profile", host && v[7]);
            is(b, P.t, s.chis, "chis", host && v[8]);
            is(b, P.t, s.lyon8, "lyon8", host && v[9]);
            is(b, P.t, s.status, "status", host);
            is(b, P.t, s.ws, "ws", v[10] != 0);
          });
    } else if (k == "scores" && got == 16) {
      const unsigned g = (unsigned)v[7];
      const int cus = (int)v[10];
      const bool avg = v[12];
      pfe::Options o;
      const int64_t pass = v[11] ? in.n % chunk : chunk;
      if (pass < 1) fail("no shorter last pass", line.c_str());
      auto walk = [&](int64_t cn) {
        return [&, cn](Arena& A) {
          return pfe::pfd_scores_layout(A, in, host, g, (int)v[8], (size_t)v[9], cus, o, chunk, cn,
                                        avg, false, ki, 0, nsum);
        };
      };
      Trace full;  // the full pass: what a last pass must leave in place
      Arena m;
      m.trace = &full;
      walk(chunk)(m);
      run(line, walk(pass), [&](const Placed& P, const pfe::PfdScoresStage& s) {
        const uintptr_t b = (uintptr_t)P.block;
        check_inputs(P, s.in, in, host, wts, chunk);
        check_avg(P, s.avg, in, host, avg, chunk);
        is(b, P.t, s.out, "out", host);
        is(b, P.t, s.status, "status", host);
        is(b, P.t, s.d22, "d22", g != pfe::PFD_G_ALL);
        is(b, P.t, s.work.profile, "profile", g == pfe::PFD_G_ALL);
        is(b, P.t, s.work.chis, "chis", (g & pfe::PFD_G_DM) != 0);
        is(b, P.t, s.work.par22, "par22", true);
        is(b, P.t, s.work.bates.ws, "gauss_ws", (g & pfe::PFD_G_DM) != 0);
        is(b, P.t, s.tg, "tg", v[9] != 0);
        for (const char* name : {"data16", "scl16", "offs16", "wts16", "subfreqs", "scal", "out",
                                 "status", "psum", "avg_csum", "avg_scal"}) {
          const Arena::Region *a = find(P.t, name), *c = find(full, name);
          if (!a != !c || (a && (a->off != c->off || a->bytes != c->bytes)))
            fail("a last pass moves", name);
        }
      });
    } else if (k == "avgprof" && got == 10) {
      const int64_t ES = (int64_t)in.npart * in.nsub, E = ES * in.proflen;
      run(line,
          [&](Arena& A) { return pfe::pfd_avgprof_layout(A, E, in.n, host, false, ki, ES, 0, 0, 0, nsum); },
          [&](const Placed& P, const pfe::PfdAvgStage& s) {
            const uintptr_t b = (uintptr_t)P.block;
            is(b, P.t, s.profs, "profs", false);
            is(b, P.t, s.profs32, "profs32", false);
            is(b, P.t, s.data16, "data16", host);
            is(b, P.t, s.scl16, "scl16", host);
            is(b, P.t, s.offs16, "offs16", host);
            is(b, P.t, s.wts16, "wts16", host && wts);
            is(b, P.t, s.out, "out", host);
            is(b, P.t, s.csum, "avg_csum", true);
            if (host) {
              touch_staged(s.data16, s.scl16, s.offs16, s.wts16, in);
              s.out[in.n - 1] = 1.0;
            }
            s.csum[(size_t)in.n * pfe::pfd_avg_chunks(E) - 1] = 1.0;
          });
    } else if (k == "scrunch" && got == 13) {
      const int64_t ES = (int64_t)in.npart * in.nsub, E = ES * in.proflen;
      const bool rot = v[7];
      const int64_t GK = (int64_t)(in.nsub / v[8]) * (in.proflen / v[9]);
      run(line,
          [&](Arena& A) {
            return pfe::pfd_scrunch_layout(A, E, ES, in.nsub, GK, in.n, host, false, ki, rot, nsum);
          },
          [&](const Placed& P, const pfe::PfdScrunchStage& s) {
            const uintptr_t b = (uintptr_t)P.block;
            is(b, P.t, s.profs, "profs", false);
            is(b, P.t, s.profs32, "profs32", false);
            is(b, P.t, s.data16, "data16", host);
            is(b, P.t, s.scl16, "scl16", host);
            is(b, P.t, s.offs16, "offs16", host);
            is(b, P.t, s.wts16, "wts16", host && wts);
            is(b, P.t, s.rot, "rot", host && rot);
            is(b, P.t, s.out, "out", host);
            if (host) {
              touch_staged(s.data16, s.scl16, s.offs16, s.wts16, in);
              if (rot) s.rot[(size_t)in.n * in.nsub - 1] = 1;
              s.out[(size_t)in.n * GK - 1] = 1.0;
            }
          });
    } else {
      return 66;
    }
  }
  fclose(f);
  puts("done");
  return 0;
}
