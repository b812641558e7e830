// pfd_scrunch_layout_driver.cpp — stand-alone check of the scratch of the pfe_pfd_scrunch calls
// (csrc/launch.h: pfd_scrunch_layout, and the route rule pfd_scrunch_lds / pfd_scrunch_slab_chans)
// on a CPU, built with ASan + UBSan by tests/test_pfd_scrunch_layout_host.py.
//
// Each line of the case file (argv[1]) is
//   n npart nchan nbin fscr bscr host form rot
// form: 0 doubles, 1 floats, 2 int16, 3 int16 with weights; rot: a rotation array is given.  The
// driver measures the layout (Arena{}), allocates exactly that many bytes, places (Arena{block}),
// fills every region over its whole length with a byte value of its own and reads all of them
// back (ASan sees an overrun, the read-back an overlap), checks each pointer of the returned
// struct against the region it is named for and the order cube, rot, out, writes each staged
// array at the last element a kernel indexes, and prints the route (lds 0/1, the channels of a
// slab, the LDS bytes of a block), `name bytes` per region and the total.  A failed check exits
// with status 2.
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
    const int64_t n = v[0];
    const int npart = (int)v[1], nchan = (int)v[2], nbin = (int)v[3], fscr = (int)v[4], bscr = (int)v[5];
    const bool host = v[6], rot = v[8];
    const int form = (int)v[7];
    if (n < 1 || npart < 1 || nchan % fscr || nbin % bscr || form < 0 || form > 3) fail("case", line.c_str());
    const int i16 = form == 2 ? pfe::PFD_I16_PLAIN : form == 3 ? pfe::PFD_I16_WEIGHTS : pfe::PFD_I16_NONE;
    const int64_t ES = (int64_t)npart * nchan, E = ES * nbin;
    const int G = nchan / fscr, K = nbin / bscr;
    const int64_t GK = (int64_t)G * K;
    // the route: what a block of the LDS kernel asks for stays within 64 KB
    const bool lds = pfe::pfd_scrunch_lds(nbin, bscr);
    const int C = pfe::pfd_scrunch_slab_chans(nbin, fscr);
    if (C < 1 || C > fscr) fail("slab channels", line.c_str());
    const size_t lds_bytes =
        lds ? ((((size_t)C * nbin + 3) & ~(size_t)3) + (C < fscr ? (size_t)K : 0)) * sizeof(double) : 0;
    if (lds_bytes > 65536) fail("a block's LDS beyond 64 KB", line.c_str());
    if (lds && C > 1 && (int64_t)C * nbin > pfe::PFD_SCR_SLAB_DOUBLES) fail("slab beyond its budget", line.c_str());
    printf("case %s\nroute %d %d %zu\n", line.c_str(), (int)lds, C, lds_bytes);

    auto walk = [&](Arena& A) {
      return pfe::pfd_scrunch_layout(A, E, ES, nchan, GK, n, host, form == 1, i16, rot);
    };
    Trace tm, tp;
    Arena m;
    m.trace = &tm;
    walk(m);
    const size_t total = m.bytes();
    unsigned char* block = total ? (unsigned char*)aligned_alloc(256, total) : nullptr;
    if (total && !block) fail("aligned_alloc", line.c_str());
    Arena pl{(uintptr_t)block};
    pl.trace = &tp;
    const pfe::PfdScrunchStage s = walk(pl);
    if (pl.bytes() != total || tp.size() != tm.size()) fail("measure and place disagree", line.c_str());
    for (size_t i = 0; i < tp.size(); ++i) {
      const Arena::Region &a = tp[i], &b = tm[i];
      if (a.off != b.off || a.bytes != b.bytes || strcmp(a.name, b.name))
        fail("measure and place disagree", a.name);
      if (a.off % 256 || a.off + a.bytes > total) fail("region out of the block", a.name);
    }
    for (size_t i = 0; i < tp.size(); ++i)
      if (tp[i].bytes) memset(block + tp[i].off, (int)(i % 251 + 1), tp[i].bytes);
    for (size_t i = 0; i < tp.size(); ++i) {  // every byte still the region's own
      const unsigned char* r = block + tp[i].off;
      if (tp[i].bytes && (r[0] != (unsigned char)(i % 251 + 1) || memcmp(r, r + 1, tp[i].bytes - 1)))
        fail("regions overlap", tp[i].name);
    }
    if (!host && (total || !tp.empty())) fail("a device-pointer call takes no scratch", line.c_str());
    const uintptr_t b = (uintptr_t)block;
    is(b, tp, s.profs, "profs", host && form == 0);
    is(b, tp, s.profs32, "profs32", host && form == 1);
    is(b, tp, s.data16, "data16", host && form >= 2);
    is(b, tp, s.scl16, "scl16", host && form >= 2);
    is(b, tp, s.offs16, "offs16", host && form >= 2);
    is(b, tp, s.wts16, "wts16", host && form == 3);
    is(b, tp, s.rot, "rot", host && rot);
    is(b, tp, s.out, "out", host);
    if (host) {
      // the cube first, out last, rot directly in front of out
      const char* first = form == 0 ? "profs" : form == 1 ? "profs32" : "data16";
      if (strcmp(tp.front().name, first) || strcmp(tp.back().name, "out")) fail("order", line.c_str());
      if (rot && strcmp(tp[tp.size() - 2].name, "rot")) fail("order", "rot");
      // the last element each kernel indexes
      if (form == 0) s.profs[(size_t)n * E - 1] = 1.0;
      if (form == 1) s.profs32[(size_t)n * E - 1] = 1.0f;
      if (form >= 2) {
        pfe_pfd_i16_in in{};
        in.data = s.data16, in.scl = s.scl16, in.offs = s.offs16, in.wts = s.wts16;
        in.npart = npart, in.nsub = nchan, in.proflen = nbin, in.n = n;
        const pfe::PfdI16Src q = pfe::pfd_i16_src(in, false).from(n - 1);
        char* d = const_cast<char*>(q.data) + (npart - 1) * q.dps + 2 * ((int64_t)nchan * nbin - 1);
        if (d + 2 != (char*)(s.data16 + (size_t)n * E)) fail("last value", "data16");
        *reinterpret_cast<int16_t*>(d) = 1;
        const int64_t at = (npart - 1) * q.pps + 4 * (int64_t)(nchan - 1);
        if (q.scl + at + 4 != (const char*)(s.scl16 + (size_t)n * ES)) fail("last value", "scl16");
        *reinterpret_cast<float*>(const_cast<char*>(q.scl) + at) = 1.0f;
        *reinterpret_cast<float*>(const_cast<char*>(q.offs) + at) = 1.0f;
        if (form == 3) *reinterpret_cast<float*>(const_cast<char*>(q.wts) + at) = 1.0f;
      }
      if (rot) s.rot[(size_t)n * nchan - 1] = 1;
      s.out[(size_t)n * GK - 1] = 1.0;
    }
    for (const Arena::Region& r : tp) printf("%s %zu\n", r.name, r.bytes);
    printf("total %zu\n", total);
    free(block);
  }
  fclose(f);
  puts("done");
  return 0;
}
