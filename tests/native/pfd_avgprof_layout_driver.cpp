// pfd_avgprof_layout_driver.cpp — stand-alone check of the scratch of pfe_pfd_avgprof and of
// PFE_FLAG_PFD_AVGPROF on the PFD calls (csrc/launch.h: pfd_avgprof_layout, pfd_avg_work_layout
// and the `avgprof` forms of pfd_dmprof_layout and pfd_scores_layout) on a CPU, built with
// ASan + UBSan by tests/test_pfd_avgprof_host.py.
//
// Each line of the case file (argv[1]) is one of
//   avgprof n npart nsub L host f32
//   dmprof  n npart nsub L host f32 opt ws_bytes
//   scores  n npart nsub L host f32 opt groups k tail
// f32 = 1: the float32 form, in passes of pfd_f32_chunk(opt) folds; tail = 1: the layout of the
// shorter last pass (n % chunk folds).  For a PFD call the driver walks the layout without the
// flag (printed as `base name bytes`) and with it.  Each walk is measured (Arena{}), allocated
// exactly, placed (Arena{block}), every region filled over its whole length with a byte value
// of its own and read back (ASan sees an overrun, the read-back an overlap); the pointers of
// the new regions are checked against the regions they are named for and written at the last
// element a kernel touches.  For a last pass the new regions must lie where the full pass has
// them.  Prints `folds`, `name bytes` per region and the total.  A failed check exits with 2.
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
static void run(const std::string& line, const char* prefix, Walk walk, Check check) {
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
  for (const Arena::Region& r : P.t) printf("%s%s %zu\n", prefix, r.name, r.bytes);
  printf("%stotal %zu\n", prefix, P.total);
  free(P.block);
}

// the two regions of the flag: the pointers, and the last element each kernel touches
static void check_avg(const Placed& P, const pfe::PfdAvgWork& w, const pfe_pfd_in& v, bool host,
                      int64_t folds) {
  const uintptr_t b = (uintptr_t)P.block;
  is(b, P.t, w.csum, "avg_csum", true);
  is(b, P.t, w.scal, "avg_scal", !host);
  const int64_t E = (int64_t)v.npart * v.nsub * v.proflen;
  w.csum[(size_t)folds * pfe::pfd_avg_chunks(E) - 1] = 1.0;
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
    long long v[10] = {};
    const int got = sscanf(buf, "%15s %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", kind, v, v + 1,
                           v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9);
    const std::string k(kind);
    pfe_pfd_in in{};
    in.n = v[0], in.npart = (int)v[1], in.nsub = (int)v[2], in.proflen = (int)v[3];
    const bool host = v[4], f32 = v[5];
    const int64_t E = (int64_t)in.npart * in.nsub * in.proflen;
    printf("case %s\n", line.c_str());
    if (k == "avgprof" && got == 7) {
      printf("folds %lld\n", (long long)in.n);
      run(line, "", [&](Arena& A) { return pfe::pfd_avgprof_layout(A, E, in.n, host, f32); },
          [&](const Placed& P, const pfe::PfdAvgStage& s) {
            const uintptr_t b = (uintptr_t)P.block;
            is(b, P.t, s.profs, "profs", host && !f32);
            is(b, P.t, s.profs32, "profs32", host && f32);
            is(b, P.t, s.out, "out", host);
            is(b, P.t, s.csum, "avg_csum", true);
            if (host && f32) s.profs32[(size_t)in.n * E - 1] = 1.0f;
            if (host && !f32) s.profs[(size_t)in.n * E - 1] = 1.0;
            if (host) s.out[(size_t)in.n - 1] = 1.0;
            s.csum[(size_t)in.n * pfe::pfd_avg_chunks(E) - 1] = 1.0;
          });
      continue;
    }
    const int64_t chunk = f32 ? pfe::pfd_f32_chunk(in.nsub, in.proflen, in.n, v[6]) : 0;
    const int64_t folds = f32 ? chunk : in.n;  // what one pass derives
    printf("folds %lld\n", (long long)folds);
    if (k == "dmprof" && got == 9) {
      auto walk = [&](bool flag) {
        return [&, flag](Arena& A) {
          return pfe::pfd_dmprof_layout(A, in, host, true, true, true, (size_t)v[7], chunk, flag);
        };
      };
      run(line, "base ", walk(false), [&](const Placed& P, const pfe::PfdDmprofStage& s) {
        const uintptr_t b = (uintptr_t)P.block;
        is(b, P.t, s.avg.csum, "avg_csum", false);
        is(b, P.t, s.avg.scal, "avg_scal", false);
      });
      run(line, "", walk(true), [&](const Placed& P, const pfe::PfdDmprofStage& s) {
        check_avg(P, s.avg, in, host, folds);
        is((uintptr_t)P.block, P.t, s.ws, "ws", v[7] != 0);
        is((uintptr_t)P.block, P.t, s.in.scal, "scal", host);
      });
    } else if (k == "scores" && got == 11) {
      const unsigned g = (unsigned)v[7];
      pfe::Options o;
      const int64_t pass = v[9] ? in.n % chunk : folds;
      if (v[9] && (!f32 || pass < 1)) fail("no shorter last pass", line.c_str());
      auto walk = [&](bool flag, int64_t cn) {
        return [&, flag, cn](Arena& A) {
          return pfe::pfd_scores_layout(A, in, host, g, (int)v[8], 0, 256, o, chunk, f32 ? cn : 0, flag);
        };
      };
      Trace full;  // the full pass: what a last pass must leave in place
      Arena m;
      m.trace = &full;
      walk(true, folds)(m);
      run(line, "base ", walk(false, pass), [&](const Placed& P, const pfe::PfdScoresStage& s) {
        const uintptr_t b = (uintptr_t)P.block;
        is(b, P.t, s.avg.csum, "avg_csum", false);
        is(b, P.t, s.avg.scal, "avg_scal", false);
      });
      run(line, "", walk(true, pass), [&](const Placed& P, const pfe::PfdScoresStage& s) {
        check_avg(P, s.avg, in, host, folds);
        is((uintptr_t)P.block, P.t, s.work.par22, "par22", true);
        for (const char* name : {"scal", "psum", "avg_csum", "avg_scal"}) {
          const Arena::Region *a = find(P.t, name), *c = find(full, name);
          if (!a != !c || (a && (a->off != c->off || a->bytes != c->bytes)))
            fail("a last pass moves", name);
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
