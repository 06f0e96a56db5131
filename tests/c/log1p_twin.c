/* The device's pmx_log1p (parmmg_amd/csrc/pmx_metric.h) in plain C: glibc's
 * log1p algorithm (sysdeps/ieee754/dbl-64/s_log1p.c, Sun's fdlibm with the
 * pairwise polynomial) -- compared bit for bit with the host's log1p by
 * tests/test_oracle.py (test infrastructure).  Build: -O2 -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static int32_t hiw(double x) { uint64_t u; memcpy(&u, &x, 8); return (int32_t)(u >> 32); }
static double sethi(double x, int32_t h) {
  uint64_t u; memcpy(&u, &x, 8);
  u = (u & 0xffffffffull) | ((uint64_t)(uint32_t)h << 32);
  memcpy(&x, &u, 8);
  return x;
}

static double twin_log1p(double x) {
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  const double Lp1 = 6.666666666666735130e-01, Lp2 = 3.999999999940941908e-01, Lp3 = 2.857142874366239149e-01,
               Lp4 = 2.222219843214978396e-01, Lp5 = 1.818357216161805012e-01, Lp6 = 1.531383769920937332e-01,
               Lp7 = 1.479819860511658591e-01;
  double f = 0.0, c = 0.0, u, hfsq, s, z, R, dk;
  int32_t hx = hiw(x), hu = 0, k = 1, ax = hx & 0x7fffffff;
  if (hx < 0x3FDA827A) {
    if (ax >= 0x3ff00000) return x == -1.0 ? -INFINITY : (x - x) / (x - x);
    if (ax < 0x3e200000) return ax < 0x3c900000 ? x : x - x * x * 0.5;
    if (hx > 0 || hx <= (int32_t)0xbfd2bec3) { k = 0; f = x; hu = 1; }
  } else if (hx >= 0x7ff00000) {
    return x + x;
  }
  if (k != 0) {
    if (hx < 0x43400000) {
      u = 1.0 + x; hu = hiw(u); k = (hu >> 20) - 1023;
      c = (k > 0) ? 1.0 - (u - x) : x - (u - 1.0);
      c /= u;
    } else {
      u = x; hu = hiw(u); k = (hu >> 20) - 1023; c = 0.0;
    }
    hu &= 0x000fffff;
    if (hu < 0x6a09e) u = sethi(u, hu | 0x3ff00000);
    else { k += 1; u = sethi(u, hu | 0x3fe00000); hu = (0x00100000 - hu) >> 2; }
    f = u - 1.0;
  }
  hfsq = 0.5 * f * f;
  dk = (double)k;
  if (hu == 0) {
    if (f == 0.0) {
      if (k == 0) return 0.0;
      c += dk * ln2_lo;
      return dk * ln2_hi + c;
    }
    R = hfsq * (1.0 - 0.66666666666666666 * f);
    if (k == 0) return f - R;
    return dk * ln2_hi - ((R - (dk * ln2_lo + c)) - f);
  }
  s = f / (2.0 + f);
  z = s * s;
  {
    double R1 = z * Lp1, z2 = z * z, R2 = Lp2 + z * Lp3, z4 = z2 * z2, R3 = Lp4 + z * Lp5, z6 = z4 * z2,
           R4 = Lp6 + z * Lp7;
    R = R1 + z2 * R2 + z4 * R3 + z6 * R4;
  }
  if (k == 0) return f - (hfsq - s * (hfsq + R));
  return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + (dk * ln2_lo + c))) - f);
}

int main(void) {
  uint64_t st = 88172645463325252ull;
  long n = 0, bad = 0, i;
  for (i = 0; i < 4000000; i++) {
    double x, r, a;
    st ^= st << 13; st ^= st >> 7; st ^= st << 17;
    switch (i % 4) {
      case 0: x = ((double)(st >> 11) / 9007199254740992.0) * 1.5 - 0.49; break;   /* h2/h1 - 1 */
      case 1: x = ((double)(st >> 11) / 9007199254740992.0) * 1e-3 - 5e-4; break;
      case 2: x = exp(((double)(st >> 11) / 9007199254740992.0) * 60 - 40); break;
      default: x = ((double)(st >> 11) / 9007199254740992.0) * 20 - 0.999; break;
    }
    r = log1p(x);
    a = twin_log1p(x);
    n++;
    if (memcmp(&a, &r, 8)) bad++;
  }
  printf("%ld %ld\n", n, bad);
  return bad != 0;
}
