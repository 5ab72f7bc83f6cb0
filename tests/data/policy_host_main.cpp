// The numpy action stream of csrc/rmx_learn.h (learn_policy_numpy) as a stand-alone program, for the sanitizer build of
// tests/test_policy_cpu.py: 200 generators (odd increments; every other one with a buffered half of 0, which forces
// Lemire's redraw on a three-way tie) x 500 choices over rows with 4, 3, 3, 2 and 1 maxima and a NaN maximum, at
// epsilon 0, 0.5 and 1.  Prints an FNV-1a digest of the actions and the final generator words; the test computes the
// same digest with tests/policyref.py.
#include <cmath>
#include <cstdio>

#include "rmx_learn.h"

using namespace rmx;

int main() {
  const double rows[6][4] = {{1, 1, 1, 1}, {0.5, 2, 2, 2}, {3, 0, 3, 3}, {1, 1, 0, -1}, {0, 0, 0, 0.5}, {NAN, 1, 2, 0}};
  uint64_t d = 0xcbf29ce484222325ull;
  for (uint64_t s = 0; s < 200; ++s) {
    LearnRng r = {s * 0x9E3779B97F4A7C15ull, ~s, s, (s << 1) | 1, (uint32_t)(s & 1), 0u};
    for (int i = 0; i < 500; ++i) {
      const double* w = rows[(s + i) % 6];
      const int a = learn_policy_numpy(r, (i % 3) * 0.5, w[0], w[1], w[2], w[3]);
      d = (d ^ (uint64_t)a) * 0x100000001b3ull;
    }
    d = (d ^ r.hi ^ r.lo ^ learn_rng_word4(r)) * 0x100000001b3ull;
  }
  printf("POLICY_HOST_DIGEST %016llx\n", (unsigned long long)d);
  return 0;
}
