// Prints the lattice step's launch plan (csrc/mfgp_lat_plan.h, the header the library's
// step engine plans with) for the cases on the command line; built and read by
// tests/test_lattice_wunits.py. Host C++ only.
//   plan:NCU:B:N0:K:M:ES:NX:NY:SF   B equal GPs, no override knobs ->
//       "plan take=T ka=A g2=G ksplit=S tiles=T wu_total=W nwu=U" (nwu: each GP's share)
//   share:TOTAL:N0,N0,...           the GPs' shares of TOTAL w units -> "share U U ..."
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mfgp_lat_plan.h"

using namespace mfgp_lat_plan;

static std::vector<long long> numbers(const char* s, const char* seps) {
  std::vector<long long> v;
  for (const char* p = s; *p;) {
    char* e = nullptr;
    v.push_back(std::strtoll(p, &e, 10));
    if (e == p) std::exit(2);
    p = e;
    while (*p && std::strchr(seps, *p)) ++p;
  }
  return v;
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    if (!std::strncmp(argv[a], "plan:", 5)) {
      const std::vector<long long> v = numbers(argv[a] + 5, ":");
      if (v.size() != 9) return 2;
      const Knobs kn = {(int)v[0], -1, false, false, 0, 0};
      const std::vector<Gp> g((size_t)v[1], Gp{v[2], v[3], v[4], (int)v[5], (int)v[6], (int)v[7], v[8] != 0});
      const Plan p = plan(kn, g.data(), (int)g.size());
      std::printf("plan take=%d ka=%d g2=%d ksplit=%d tiles=%lld wu_total=%lld nwu=%d\n", p.take ? 1 : 0, p.ka,
                  p.g2 ? 1 : 0, p.ksplit, (long long)p.tiles_sum, (long long)p.wu_total,
                  p.take ? w_share(p.wu_total, p.wsteps_sum, g[0].n0) : 0);
    } else if (!std::strncmp(argv[a], "share:", 6)) {
      const std::vector<long long> v = numbers(argv[a] + 6, ":,");
      if (v.size() < 2) return 2;
      long long sum = 0;
      for (size_t i = 1; i < v.size(); ++i) sum += wsteps(v[i]);
      std::printf("share");
      for (size_t i = 1; i < v.size(); ++i) std::printf(" %d", w_share(v[0], sum, v[i]));
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
