// subband_f64_layout_driver.cpp — stand-alone check of the scratch of pfe_subband3_f64 and
// pfe_bates22_f64 (csrc/launch.h: subf64_plan, subband_f64_layout) on a CPU, built with
// ASan + UBSan by tests/test_subband_f64_layout_host.py.
//
// Each line of the case file (argv[1]) is `n lp nsub lsb ndm host chain force_global cus`.
// The driver plans the launch, measures the layout (Arena{}), allocates exactly that many
// bytes, places (Arena{block}), fills every region over its whole length with a byte value of
// its own and reads all of them back (ASan sees an overrun, the read-back an overlap), checks
// each pointer of the returned struct against the region it is named for, writes every wave's
// slab over its whole length, and prints the plan, `name bytes` per region and the total.  A
// failed check exits with status 2.
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

int main(int argc, char** argv) {
  if (argc != 2) return 64;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 65;
  char buf[256];
  while (fgets(buf, sizeof(buf), f)) {
    std::string line(buf);
    while (!line.empty() && (line.back() == '\n' || line.back() == ' ')) line.pop_back();
    if (line.empty()) continue;
    long long v[9] = {};
    if (sscanf(buf, "%lld %lld %lld %lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4, v + 5,
               v + 6, v + 7, v + 8) != 9)
      return 66;
    pfe_bates_f64_in in{};
    in.n = v[0], in.lp = (int)v[1], in.nsub = (int)v[2], in.lsb = (int)v[3], in.ndm = (int)v[4];
    const bool host = v[5], chain = v[6], force = v[7];
    const int cus = (int)v[8];
    pfe::Options o;
    const pfe::SubF64Plan p = pfe::subf64_plan(in.nsub, in.lsb, in.n, cus, force);
    printf("case %s\n", line.c_str());
    printf("plan %d %d %zu %zu %zu %d %d\n", (int)p.ok, (int)p.global, p.wave_lds, p.t_lds, p.slab,
           p.wpb, p.blocks);
    if (!p.ok) continue;
    auto walk = [&](Arena& A) { return pfe::subband_f64_layout(A, in, host, chain, p.slab_bytes(), cus, o); };
    Trace tm, tp;
    Arena m;
    m.trace = &tm;
    walk(m);
    const size_t total = m.bytes();
    unsigned char* block = total ? (unsigned char*)aligned_alloc(256, total) : nullptr;
    if (total && !block) fail("aligned_alloc", line.c_str());
    Arena pl{(uintptr_t)block};
    pl.trace = &tp;
    const pfe::SubF64Stage s = walk(pl);
    if (pl.bytes() != total || tp.size() != tm.size()) fail("measure and place disagree", line.c_str());
    for (size_t i = 0; i < tp.size(); ++i) {
      if (tp[i].off != tm[i].off || tp[i].bytes != tm[i].bytes || strcmp(tp[i].name, tm[i].name))
        fail("measure and place disagree", tp[i].name);
      if (tp[i].off % 256 || tp[i].off + tp[i].bytes > total) fail("region out of the block", tp[i].name);
    }
    if (block) {
      const uintptr_t b = (uintptr_t)block;
      is(b, tp, s.prof, "prof", host);
      is(b, tp, s.sub, "sub", host);
      is(b, tp, s.dmcurve, "dmcurve", host && chain);
      is(b, tp, s.scal, "scal", host);
      is(b, tp, s.out, "out", host);
      is(b, tp, s.status, "status", host);
      is(b, tp, s.bates.ws, "gauss_ws", chain);
      is(b, tp, s.bates.wscr, "wave_scratch", chain);
      is(b, tp, s.slabs, "slabs", p.global);
    }
    for (size_t i = 0; i < tp.size(); ++i)
      if (tp[i].bytes) memset(block + tp[i].off, (int)(i % 251 + 1), tp[i].bytes);
    for (size_t i = 0; i < tp.size(); ++i) {  // every byte still the region's own
      const unsigned char* r = block + tp[i].off;
      if (tp[i].bytes && (r[0] != (unsigned char)(i % 251 + 1) || memcmp(r, r + 1, tp[i].bytes - 1)))
        fail("regions overlap", tp[i].name);
    }
    if (p.global) {  // every wave's slab holds the candidate's doubles, inside the region
      const size_t need = (size_t)in.nsub * in.lsb * sizeof(double);
      if (p.slab < need || p.slab % 256) fail("slab size", line.c_str());
      for (int w = 0; w < p.wpb * p.blocks; ++w) memset((unsigned char*)s.slabs + (size_t)w * p.slab, w & 255, need);
    }
    for (const Arena::Region& r : tp) printf("%s %zu\n", r.name, r.bytes);
    printf("total %zu\n", total);
    free(block);
  }
  fclose(f);
  puts("done");
  return 0;
}
