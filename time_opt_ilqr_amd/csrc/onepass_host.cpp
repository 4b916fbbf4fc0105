// Host build of onepass_pick.hpp for the CPU test suite (not part of libhop_amd.so):
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -DHOP_HD=
//       onepass_host.cpp -o libonepass_host.so
// Runs the pick kernel's per-problem arithmetic on the CPU, problem by problem, with
// hop_onepass_pick_f64's arguments (no stream).
#include <stdint.h>

#include "onepass_pick.hpp"

using namespace hop::onepass;

template <int n>
static void run(const PickDims& d, const double* Vxx, const double* Vx, const double* V0,
                const double* X_ext, const double* x0, const int32_t* T_bar, int64_t batch,
                int32_t* T_star, double* Jw) {
  const int64_t L = d.n_ext;
  for (int64_t b = 0; b < batch; ++b)
    T_star[b] = pick_one<n>(d, Vxx + b * L * n * n, Vx + b * L * n, V0 + b * L, X_ext + b * L * n,
                            x0 + b * n, T_bar[b], Jw + b * d.T_max);
}

extern "C" int onepass_host_pick(const double* Vxx, const double* Vx, const double* V0,
                                 const double* X_ext, const double* x0, const int32_t* T_bar,
                                 int64_t batch, int32_t n, int32_t n_ext, int32_t T_min,
                                 int32_t T_max, int32_t S_left, int32_t S_right,
                                 uint32_t wrap_mask, double locality_mult, int32_t* T_star,
                                 double* Jw) {
  if (n_ext < 1 || T_min < 1 || T_max < T_min || S_left < 0 || S_right < 0 ||
      S_left > kMaxWindow || S_right > kMaxWindow)
    return -1;
  const PickDims d{n_ext, T_min, T_max, S_left, S_right, wrap_mask, locality_mult};
  switch (n) {
    case 2: run<2>(d, Vxx, Vx, V0, X_ext, x0, T_bar, batch, T_star, Jw); return 0;
    case 4: run<4>(d, Vxx, Vx, V0, X_ext, x0, T_bar, batch, T_star, Jw); return 0;
    case 12: run<12>(d, Vxx, Vx, V0, X_ext, x0, T_bar, batch, T_star, Jw); return 0;
    default: return -2;
  }
}
