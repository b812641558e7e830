// cand_f32_layout_driver.cpp — stand-alone check of the scratch of the float32 forms of the
// float-array calls (csrc/launch.h: subband_f32_layout, the f32 form of group_layout and
// lyon8_slot_layout<float>) on a CPU, built with ASan + UBSan by
// tests/test_cand_f32_layout_host.py.
//
// Each line of the case file (argv[1]) is one of
//   score n lp nsub lsb ndm host chain global cus
//   group n lp groups k host cus
//   lyon8 chunk lp ld
// global: PFE_OPT_SUBF64_GLOBAL.  The driver plans the sub-band kernel (subf64_plan: the copy is
// doubles whatever the input), measures the layout (Arena{}), allocates exactly that many bytes,
// places (Arena{block}), fills every region over its whole length with a byte value of its own
// and reads all of them back (ASan sees an overrun, the read-back an overlap), checks each
// pointer of the returned struct against the region it is named for, writes the last element
// each kernel or copy touches, and prints `name bytes` per region and the total.  A failed check
// exits with status 2.
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

struct Placed {
  unsigned char* block = nullptr;
  size_t total = 0;
  Trace t;
  // p is the region `name` (taken), or null with no such region (not taken)
  void is(const void* p, const char* name, bool taken) const {
    const Arena::Region* r = find(t, name);
    if (!taken) {
      if (p || r) fail("region not asked for", name);
      return;
    }
    if (!r || p != (const void*)(block + r->off)) fail("pointer is not region", name);
  }
  // the region holds `count` elements of `size` bytes, exactly
  void holds(const char* name, size_t count, size_t size) const {
    const Arena::Region* r = find(t, name);
    if (!r || r->bytes != count * size) fail("region size", name);
  }
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
    long long v[9] = {};
    const int got = sscanf(buf, "%15s %lld %lld %lld %lld %lld %lld %lld %lld %lld", kind, v, v + 1,
                           v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8);
    const std::string k(kind);
    pfe::Options o;
    printf("case %s\n", line.c_str());
    if (k == "score" && got == 10) {
      pfe_bates_f32_in in{};
      in.n = v[0], in.lp = (int)v[1], in.nsub = (int)v[2], in.lsb = (int)v[3], in.ndm = (int)v[4];
      const bool host = v[5], chain = v[6];
      const int cus = (int)v[8];
      const pfe::SubF64Plan p = pfe::subf64_plan(in.nsub, in.lsb, in.n, cus, v[7] != 0);
      if (!p.ok) fail("plan", line.c_str());
      printf("slab %zu\n", p.slab_bytes());
      run(line,
          [&](Arena& A) { return pfe::subband_f32_layout(A, in, host, chain, p.slab_bytes(), cus, o); },
          [&](const Placed& P, const pfe::SubF32Stage& s) {
            const size_t n = (size_t)in.n;
            P.is(s.prof, "prof", host);
            P.is(s.sub, "sub", host);
            P.is(s.dmcurve, "dmcurve", host && chain);
            P.is(s.scal, "scal", host);
            P.is(s.out, "out", host);
            P.is(s.status, "status", host);
            P.is(s.fprof, "fprof", chain);
            P.is(s.fdm, "fdm", chain);
            P.is(s.bates.ws, "gauss_ws", chain);
            P.is(s.slabs, "slabs", p.slab_bytes() != 0);
            if (host) {  // staged as the floats they are
              P.holds("prof", n * in.lp, sizeof(float));
              P.holds("sub", n * in.nsub * in.lsb, sizeof(float));
              s.prof[n * in.lp - 1] = 1.0f;
              s.sub[n * in.nsub * in.lsb - 1] = 1.0f;
              s.scal[n * PFE_NSCAL - 1] = 1.0;
              s.out[n * (chain ? 22 : 3) - 1] = 1.0;
              s.status[n - 1] = 1u;
              if (chain) {
                P.holds("dmcurve", n * in.ndm, sizeof(float));
                s.dmcurve[n * in.ndm - 1] = 1.0f;
              }
            }
            if (chain) {  // the widened copies k_widen_f32 writes and the fits read
              P.holds("fprof", n * in.lp, sizeof(double));
              P.holds("fdm", n * in.ndm, sizeof(double));
              s.fprof[n * in.lp - 1] = 1.0;
              s.fdm[n * in.ndm - 1] = 1.0;
            }
            if (p.slab_bytes()) {  // the last double of the last wave's copy of a candidate
              double* T = reinterpret_cast<double*>((unsigned char*)s.slabs +
                                                    ((size_t)p.blocks * p.wpb - 1) * p.slab);
              T[(size_t)in.nsub * in.lsb - 1] = 1.0;
            }
          });
    } else if (k == "group" && got == 7) {
      const unsigned g = (unsigned)v[2];
      const bool host = v[4];
      run(line,
          [&](Arena& A) {
            return pfe::group_layout(A, v[0], (int)v[1], 0, g, true, (int)v[3], host, (int)v[5], o, true);
          },
          [&](const Placed& P, const pfe::GroupStage& s) {
            const size_t n = (size_t)v[0], lp = (size_t)v[1];
            P.is(s.prof32, "prof32", host);
            P.is(s.fprof, "fprof", true);  // host pointers or device
            P.is(s.prof, "prof", false);
            P.is(s.dmcurve, "dmcurve", false);
            P.is(s.scal, "scal", false);
            P.is(s.d22, "d22", true);
            P.is(s.out, "out", host);
            P.is(s.status, "status", host);
            P.is(s.bates.ws, "gauss_ws", true);
            P.holds("fprof", n * lp, sizeof(double));
            s.fprof[n * lp - 1] = 1.0;
            s.d22[n * 22 - 1] = 1.0;
            if (host) {
              P.holds("prof32", n * lp, sizeof(float));
              s.prof32[n * lp - 1] = 1.0f;
              s.out[n * (size_t)v[3] - 1] = 1.0;
            }
          });
    } else if (k == "lyon8" && got == 4) {
      run(line, [&](Arena& A) { return pfe::lyon8_slot_layout<float>(A, v[0], (int)v[1], (int)v[2]); },
          [&](const Placed& P, const pfe::Lyon8Slot<float>& s) {
            P.is(s.prof, "prof", true);
            P.is(s.dm, "dm", true);
            P.is(s.out, "out", true);
            s.prof[(size_t)v[0] * v[1] - 1] = 1.0f;
            s.dm[(size_t)v[0] * v[2] - 1] = 1.0f;
            s.out[(size_t)v[0] * 8 - 1] = 1.0;
          });
    } else {
      return 66;
    }
  }
  fclose(f);
  puts("done");
  return 0;
}
