// pfd_kill_layout_driver.cpp — stand-alone check of the scratch of the pfe_pfd_*_kill calls
// (csrc/launch.h: pfd_f32_chunk and the masked forms of pfd_dmprof_layout, pfd_scores_layout and
// pfd_avgprof_layout) on a CPU, built with ASan + UBSan by tests/test_pfd_kill_layout_host.py.
//
// Each line of the case file (argv[1]) is one of
//   dmprof n npart nsub L host opt f32 kill profile chis lyon8 ws_bytes avgprof
//   scores n npart nsub L host opt f32 kill groups k g_bytes cus tail avgprof
//   avgprof n npart nsub L host 0 f32 kill
// opt: PFE_OPT_PFD_F32_CHUNK; f32: a float32 cube; kill: 1 parts, 2 subs, 3 both; tail = 1: the
// layout of the shorter last pass (n % chunk folds); avgprof: PFE_FLAG_PFD_AVGPROF.  The driver
// sizes the pass (pfd_f32_chunk), measures the layout (Arena{}), allocates exactly that many
// bytes, places (Arena{block}), fills every region over its whole length with a byte value of its
// own and reads all of them back (ASan sees an overrun, the read-back an overlap), checks each
// pointer of the returned struct against the region it is named for, writes the staged arrays,
// the masks (through PfdKillSrc::from, at the last fold of the last pass) and the part sums at the
// last element the kernels index, and prints the chunk, `name bytes` per region and the total.
// For a last pass it also checks that the staged arrays, the masks and the part sums lie where
// the full pass has them.  A failed check exits with status 2.
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

// region `b` lies directly behind region `a`: nothing is taken between them
static void behind(const Trace& t, const char* a, const char* b) {
  for (size_t i = 0; i + 1 < t.size(); ++i)
    if (!strcmp(t[i].name, a)) {
      if (strcmp(t[i + 1].name, b)) fail("not directly behind its predecessor", b);
      return;
    }
  fail("region missing", a);
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

// the staged masks as a pass reaches them: the masks of the last fold, its last part and sub-band
static void touch_masks(uint8_t* kparts, uint8_t* ksubs, const pfe_pfd_in& v, int kill) {
  pfe::PfdKillSrc k;
  k.parts = kparts;
  k.subs = ksubs;
  if (k.mask() != kill) fail("mask bits", "kill");
  const pfe::PfdKillSrc last = k.from(v.n - 1, v.npart, v.nsub);
  if (kparts) {
    if (last.parts + v.npart != kparts + (size_t)v.n * v.npart) fail("masks of a pass", "kill_parts");
    const_cast<uint8_t*>(last.parts)[v.npart - 1] = 1;
  } else if (last.parts) {
    fail("a null mask advanced", "kill_parts");
  }
  if (ksubs) {
    if (last.subs + v.nsub != ksubs + (size_t)v.n * v.nsub) fail("masks of a pass", "kill_subs");
    const_cast<uint8_t*>(last.subs)[v.nsub - 1] = 1;
  } else if (last.subs) {
    fail("a null mask advanced", "kill_subs");
  }
}

// the staged arrays, the masks and the part sums: the pointers, and the last element each kernel
// touches
static void check_inputs(const Placed& P, const pfe::PfdInputs& in, const pfe_pfd_in& v, bool host,
                         bool f32, int kill, int64_t chunk) {
  const uintptr_t b = (uintptr_t)P.block;
  is(b, P.t, in.profs, "profs", host && !f32);
  is(b, P.t, in.profs32, "profs32", host && f32);
  is(b, P.t, in.data16, "data16", false);
  is(b, P.t, in.subfreqs, "subfreqs", host);
  is(b, P.t, in.scal, "scal", host);
  is(b, P.t, in.kparts, "kill_parts", host && (kill & pfe::PFD_KILL_PARTS));
  is(b, P.t, in.ksubs, "kill_subs", host && (kill & pfe::PFD_KILL_SUBS));
  is(b, P.t, in.psum, "psum", true);
  const size_t E = (size_t)v.nsub * v.proflen, cube = (size_t)v.n * v.npart * E;
  if (host) {
    if (f32)
      in.profs32[cube - 1] = 1.0f;
    else
      in.profs[cube - 1] = 1.0;
    // directly behind scal: parts then subs, each only when given
    const char* prev = "scal";
    if (kill & pfe::PFD_KILL_PARTS) behind(P.t, prev, "kill_parts"), prev = "kill_parts";
    if (kill & pfe::PFD_KILL_SUBS) behind(P.t, prev, "kill_subs");
    touch_masks(in.kparts, in.ksubs, v, kill);
  }
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
    long long v[14] = {};
    const int got = sscanf(buf, "%15s %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld",
                           kind, v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9,
                           v + 10, v + 11, v + 12, v + 13);
    const std::string k(kind);
    pfe_pfd_in in{};
    in.n = v[0], in.npart = (int)v[1], in.nsub = (int)v[2], in.proflen = (int)v[3];
    const bool host = v[4], f32 = v[6];
    const int kill = (int)v[7];
    if (kill < 1 || kill > 3) fail("a masked call has a mask", line.c_str());
    const int64_t chunk = pfe::pfd_f32_chunk(in.nsub, in.proflen, in.n, v[5]);
    if (chunk < 1 || chunk > in.n) fail("chunk", line.c_str());
    if ((size_t)chunk * in.nsub * in.proflen * sizeof(double) > pfe::PFD_F32_PSUM_BUDGET && chunk != 1)
      fail("part sums beyond the budget", line.c_str());
    printf("case %s\nchunk %lld\n", line.c_str(), (long long)chunk);
    if (k == "dmprof" && got == 14) {
      const bool avg = v[12];
      run(line,
          [&](Arena& A) {
            return pfe::pfd_dmprof_layout(A, in, host, v[8], v[9], v[10], (size_t)v[11], chunk, avg,
                                          !f32, pfe::PFD_I16_NONE, kill);
          },
          [&](const Placed& P, const pfe::PfdDmprofStage& s) {
            const uintptr_t b = (uintptr_t)P.block;
            check_inputs(P, s.in, in, host, f32, kill, chunk);
            check_avg(P, s.avg, in, host, avg, chunk);
            is(b, P.t, s.profile, "profile", host && v[8]);
            is(b, P.t, s.chis, "chis", host && v[9]);
            is(b, P.t, s.lyon8, "lyon8", host && v[10]);
            is(b, P.t, s.status, "status", host);
            is(b, P.t, s.ws, "ws", v[11] != 0);
          });
    } else if (k == "scores" && got == 15) {
      const unsigned g = (unsigned)v[8];
      const int cus = (int)v[11];
      const bool avg = v[13];
      pfe::Options o;
      const int64_t pass = v[12] ? in.n % chunk : chunk;
      if (pass < 1) fail("no shorter last pass", line.c_str());
      auto walk = [&](int64_t cn) {
        return [&, cn](Arena& A) {
          return pfe::pfd_scores_layout(A, in, host, g, (int)v[9], (size_t)v[10], cus, o, chunk, cn,
                                        avg, !f32, pfe::PFD_I16_NONE, kill);
        };
      };
      Trace full;  // the full pass: what a last pass must leave in place
      Arena m;
      m.trace = &full;
      walk(chunk)(m);
      run(line, walk(pass), [&](const Placed& P, const pfe::PfdScoresStage& s) {
        const uintptr_t b = (uintptr_t)P.block;
        check_inputs(P, s.in, in, host, f32, kill, chunk);
        check_avg(P, s.avg, in, host, avg, chunk);
        is(b, P.t, s.out, "out", host);
        is(b, P.t, s.status, "status", host);
        is(b, P.t, s.d22, "d22", g != pfe::PFD_G_ALL);
        is(b, P.t, s.work.profile, "profile", g == pfe::PFD_G_ALL);
        is(b, P.t, s.work.chis, "chis", (g & pfe::PFD_G_DM) != 0);
        is(b, P.t, s.work.par22, "par22", true);
        is(b, P.t, s.work.bates.ws, "gauss_ws", (g & pfe::PFD_G_DM) != 0);
        is(b, P.t, s.tg, "tg", v[10] != 0);
        for (const char* name : {"profs", "profs32", "subfreqs", "scal", "kill_parts", "kill_subs",
                                 "out", "status", "psum", "avg_csum", "avg_scal"}) {
          const Arena::Region *a = find(P.t, name), *c = find(full, name);
          if (!a != !c || (a && (a->off != c->off || a->bytes != c->bytes)))
            fail("a last pass moves", name);
        }
      });
    } else if (k == "avgprof" && got == 9) {
      const int64_t E = (int64_t)in.npart * in.nsub * in.proflen;
      run(line,
          [&](Arena& A) {
            return pfe::pfd_avgprof_layout(A, E, in.n, host, f32, pfe::PFD_I16_NONE, 0, kill, in.npart,
                                           in.nsub);
          },
          [&](const Placed& P, const pfe::PfdAvgStage& s) {
            const uintptr_t b = (uintptr_t)P.block;
            is(b, P.t, s.profs, "profs", host && !f32);
            is(b, P.t, s.profs32, "profs32", host && f32);
            is(b, P.t, s.data16, "data16", false);
            is(b, P.t, s.kparts, "kill_parts", host && (kill & pfe::PFD_KILL_PARTS));
            is(b, P.t, s.ksubs, "kill_subs", host && (kill & pfe::PFD_KILL_SUBS));
            is(b, P.t, s.out, "out", host);
            is(b, P.t, s.csum, "avg_csum", true);
            if (host) {
              if (f32)
                s.profs32[(size_t)in.n * E - 1] = 1.0f;
              else
                s.profs[(size_t)in.n * E - 1] = 1.0;
              const char* prev = f32 ? "profs32" : "profs";
              if (kill & pfe::PFD_KILL_PARTS) behind(P.t, prev, "kill_parts"), prev = "kill_parts";
              if (kill & pfe::PFD_KILL_SUBS) behind(P.t, prev, "kill_subs");
              touch_masks(s.kparts, s.ksubs, in, kill);
              s.out[in.n - 1] = 1.0;
            }
            s.csum[(size_t)in.n * pfe::pfd_avg_chunks(E) - 1] = 1.0;
          });
    } else {
      return 66;
    }
  }
  fclose(f);
  puts("done");
  return 0;
}
