// layout_driver.cpp — stand-alone check of the device-scratch layouts (csrc/launch.h) on a CPU,
// built with ASan + UBSan by tests/test_scratch_layout_host.py.
//
// Each line of the case file (argv[1]) names a layout and its parameters.  For each the driver
// measures (Arena{}), allocates exactly that many bytes, 256-aligned, places (Arena{block}),
// fills every region over its whole length with a byte value of its own, reads all regions
// back (ASan sees an overrun, the read-back an overlap), checks that each pointer of the
// returned struct is the region it is named for, and prints `name bytes` per region and the
// total.  A failed check exits with status 2.
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

struct Placed {
  uintptr_t base;
  const Trace* t;
  // the start of the region `name` (the `nth` of that name)
  const void* at(const char* name, int nth = 0) const {
    for (const Arena::Region& r : *t)
      if (!strcmp(r.name, name) && nth-- == 0) return (const void*)(base + r.off);
    fail("no region", name);
  }
  void is(const void* p, const char* name, bool taken = true, int nth = 0) const {
    if (!taken) {
      if (p) fail("pointer of a region not taken", name);
      for (const Arena::Region& r : *t)
        if (!strcmp(r.name, name) && nth-- == 0) fail("region not asked for", name);
      return;
    }
    if (p != at(name, nth)) fail("pointer is not region", name);
  }
};

static void check_bates(const Placed& P, const pfe::BatesArgs& a, bool handover, bool sub, int nth = 0) {
  P.is(a.ws, "gauss_ws", true, nth);
  P.is(a.counters, "counters", true, nth);
  static const char* const hn[3] = {"hand_gauss", "hand_dm", "hand_sine"};
  for (int r = 0; r < 3; ++r) {
    P.at(hn[r], nth);  // taken with or without the option
    if (handover ? a.hand[r] != P.at(hn[r], nth) : a.hand[r] != nullptr) fail("hand-over", hn[r]);
  }
  P.is(a.wide_list, "wide_list", true, nth);
  P.is(a.wide_scr, "wide_slabs", true, nth);
  P.is(a.wscr, "wave_scratch", true, nth);
  P.is(a.sub_work, "sub_work", sub, nth);
}

// measure, allocate, place, fill, read back, print
template <class Walk, class Check>
static void run(const std::string& line, Walk walk, Check check) {
  Trace tm, tp;
  Arena m;
  m.trace = &tm;
  walk(m);
  const size_t total = m.bytes();
  unsigned char* block = total ? (unsigned char*)aligned_alloc(256, total) : nullptr;
  if (total && !block) fail("aligned_alloc", line.c_str());
  Arena p{(uintptr_t)block};
  p.trace = &tp;
  auto s = walk(p);
  if (p.bytes() != total || tp.size() != tm.size()) fail("measure and place disagree", line.c_str());
  for (size_t i = 0; i < tp.size(); ++i) {
    if (tp[i].off != tm[i].off || tp[i].bytes != tm[i].bytes || strcmp(tp[i].name, tm[i].name))
      fail("measure and place disagree", tp[i].name);
    if (tp[i].off % 256 || tp[i].off + tp[i].bytes > total) fail("region out of the block", tp[i].name);
  }
  if (block) check(Placed{(uintptr_t)block, &tp}, s);
  for (size_t i = 0; i < tp.size(); ++i)
    if (tp[i].bytes) memset(block + tp[i].off, (int)(i % 251 + 1), tp[i].bytes);
  for (size_t i = 0; i < tp.size(); ++i) {  // every byte still the region's own
    const unsigned char* r = block + tp[i].off;
    if (tp[i].bytes && (r[0] != (unsigned char)(i % 251 + 1) || memcmp(r, r + 1, tp[i].bytes - 1)))
      fail("regions overlap", tp[i].name);
  }
  printf("case %s\n", line.c_str());
  for (const Arena::Region& r : tp) printf("%s %zu\n", r.name, r.bytes);
  printf("total %zu\n", total);
  free(block);
}

int main(int argc, char** argv) {
  if (argc != 2) return 64;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 65;
  char buf[512], kind[32];
  while (fgets(buf, sizeof(buf), f)) {
    std::string line(buf);
    while (!line.empty() && (line.back() == '\n' || line.back() == ' ')) line.pop_back();
    if (line.empty()) continue;
    long long v[12] = {};
    const int got = sscanf(buf, "%31s %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", kind, v,
                           v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11);
    if (got < 2) return 66;
    const std::string k(kind);
    pfe::Options o;
    if (k == "bates") {  // n lp sub_bytes cus handover
      o.handover = (int)v[4];
      run(line,
          [&](Arena& A) {
            pfe::BatesArgs a{};
            pfe::bates_layout(A, a, v[0], (int)v[1], (size_t)v[2], (int)v[3], o);
            return a;
          },
          [&](const Placed& P, const pfe::BatesArgs& a) { check_bates(P, a, v[4], v[2] != 0); });
    } else if (k == "pfd22") {  // n L groups cus handover
      o.handover = (int)v[4];
      const bool all = v[2] == pfe::PFD_G_ALL, dm = v[2] & pfe::PFD_G_DM;
      run(line, [&](Arena& A) { return pfe::pfd22_layout(A, v[0], (int)v[1], (unsigned)v[2], (int)v[3], o); },
          [&](const Placed& P, const pfe::Pfd22Work& w) {
            P.is(w.profile, "profile", all);
            P.is(w.chis, "chis", dm);
            P.is(w.par22, "par22");
            if (dm) check_bates(P, w.bates, v[4], false);
          });
    } else if (k == "score") {  // n lp nsub lsb ndm host chain sub_bytes cus handover
      pfe_bates_in in{};
      in.n = v[0], in.lp = (int)v[1], in.nsub = (int)v[2], in.lsb = (int)v[3], in.ndm = (int)v[4];
      const bool host = v[5], chain = v[6];
      o.handover = (int)v[9];
      run(line, [&](Arena& A) { return pfe::score_layout(A, in, host, chain, (size_t)v[7], (int)v[8], o); },
          [&](const Placed& P, const pfe::ScoreStage& s) {
            P.is(s.prof, "prof", host);
            P.is(s.sub, "sub", host);
            P.is(s.dmcurve, "dmcurve", host && chain);
            P.is(s.scal, "scal", host);
            P.is(s.out, "out", host);
            P.is(s.status, "status", host);
            if (chain)
              check_bates(P, s.bates, v[9], v[7] != 0);
            else
              P.is(s.sub_work, "sub_work", v[7] != 0);
          });
    } else if (k == "group") {  // n lp ndm groups f64 k host cus handover
      const unsigned g = (unsigned)v[3];
      const bool f64 = v[4], host = v[6];
      o.handover = (int)v[8];
      run(line,
          [&](Arena& A) {
            return pfe::group_layout(A, v[0], (int)v[1], (int)v[2], g, f64, (int)v[5], host, (int)v[7], o);
          },
          [&](const Placed& P, const pfe::GroupStage& s) {
            P.is(s.dmcurve, "dmcurve", host && g == pfe::BG_DM);
            P.is(s.fprof, "fprof", host && g != pfe::BG_DM && f64);
            P.is(s.prof, "prof", host && g != pfe::BG_DM && !f64 && g);
            P.is(s.scal, "scal", host && !f64);
            P.is(s.d22, "d22", g != 0);
            P.is(s.out, "out", host);
            P.is(s.status, "status", host);
            if (g) check_bates(P, s.bates, v[8], false);
          });
    } else if (k == "pfd_dmprof") {  // n npart nsub L host profile chis lyon8 ws_bytes
      pfe_pfd_in in{};
      in.n = v[0], in.npart = (int)v[1], in.nsub = (int)v[2], in.proflen = (int)v[3];
      const bool host = v[4];
      run(line, [&](Arena& A) { return pfe::pfd_dmprof_layout(A, in, host, v[5], v[6], v[7], (size_t)v[8]); },
          [&](const Placed& P, const pfe::PfdDmprofStage& s) {
            P.is(s.in.profs, "profs", host);
            P.is(s.in.subfreqs, "subfreqs", host);
            P.is(s.in.scal, "scal", host);
            P.is(s.profile, "profile", host && v[5]);
            P.is(s.chis, "chis", host && v[6]);
            P.is(s.lyon8, "lyon8", host && v[7]);
            P.is(s.status, "status", host);
            P.is(s.ws, "ws", v[8] != 0);
          });
    } else if (k == "pfd_scores") {  // n npart nsub L host groups k g_bytes cus handover
      pfe_pfd_in in{};
      in.n = v[0], in.npart = (int)v[1], in.nsub = (int)v[2], in.proflen = (int)v[3];
      const bool host = v[4];
      const unsigned g = (unsigned)v[5];
      o.handover = (int)v[9];
      run(line,
          [&](Arena& A) {
            return pfe::pfd_scores_layout(A, in, host, g, (int)v[6], (size_t)v[7], (int)v[8], o);
          },
          [&](const Placed& P, const pfe::PfdScoresStage& s) {
            P.is(s.in.profs, "profs", host);
            P.is(s.in.subfreqs, "subfreqs", host);
            P.is(s.in.scal, "scal", host);
            P.is(s.out, "out", host);
            P.is(s.status, "status", host);
            P.is(s.d22, "d22", g != pfe::PFD_G_ALL);
            P.is(s.work.profile, "profile", g == pfe::PFD_G_ALL);
            P.is(s.work.chis, "chis", (g & pfe::PFD_G_DM) != 0);
            P.is(s.work.par22, "par22");
            if (g & pfe::PFD_G_DM) check_bates(P, s.work.bates, v[9], false);
            P.is(s.tg, "tg", v[7] != 0);
          });
    } else if (k == "lyon8") {  // bytes-per-bin chunk lp ld
      auto check = [&](const Placed& P, const auto& s) {
        P.is(s.prof, "prof");
        P.is(s.dm, "dm");
        P.is(s.out, "out");
      };
      if (v[0] == 1)
        run(line, [&](Arena& A) { return pfe::lyon8_slot_layout<uint8_t>(A, v[1], (int)v[2], (int)v[3]); }, check);
      else
        run(line, [&](Arena& A) { return pfe::lyon8_slot_layout<double>(A, v[1], (int)v[2], (int)v[3]); }, check);
    } else {
      return 67;
    }
  }
  fclose(f);
  puts("done");
  return 0;
}
