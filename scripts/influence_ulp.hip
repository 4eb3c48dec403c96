// The worst error, in float32 ulps, of the three device functions the influence epilogue leans on (csrc/influence.hip: expm1f,
// log1pf, expf), against the host's double functions, over the arguments the epilogue can reach: |x| from 2^-40 to 2 for expm1f and
// log1pf (differences of logits and sums of them; log1pf from above -1/2 only), -40 <= x <= 0 for expf (log-posteriors).
// tests/influence_truth.py allots twice what this prints (profiles/influence.txt).
//   hipcc -O3 --offload-arch=gfx950 scripts/influence_ulp.hip -o influence_ulp && ./influence_ulp
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include <vector>

__global__ void k_eval(int which, const float* __restrict__ x, float* __restrict__ y, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  y[i] = which == 0 ? expm1f(x[i]) : which == 1 ? log1pf(x[i]) : expf(x[i]);
}

static double ulp_of(double v) {
  int e;
  frexp(v, &e);
  return ldexp(1.0, (e < -125 ? -125 : e) - 24);
}

int main() {
  const int count = 1 << 22;
  const char* names[3] = {"expm1f", "log1pf", "expf"};
  std::vector<float> x(count), y(count);
  float *dx, *dy;
  if (hipMalloc(&dx, count * sizeof(float)) != hipSuccess || hipMalloc(&dy, count * sizeof(float)) != hipSuccess) return 1;
  for (int which = 0; which < 3; ++which) {
    unsigned long long s = 0x9E3779B97F4A7C15ull + which;
    for (int i = 0; i < count; ++i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const double r = (double)(s >> 11) / 9007199254740992.0;      // [0, 1)
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const double q = (double)(s >> 11) / 9007199254740992.0;
      if (which == 2) {
        x[i] = (float)(-40.0 * r);
      } else {
        const double mag = ldexp(1.0 + q, -40 + (int)(r * 41.0));    // 2^-40 .. 2
        const bool neg = (s >> 7) & 1;
        x[i] = (float)(neg ? -(which == 1 && mag > 0.5 ? 0.5 * q : mag) : mag);
      }
    }
    if (hipMemcpy(dx, x.data(), count * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return 1;
    k_eval<<<(count + 255) / 256, 256>>>(which, dx, dy, count);
    if (hipMemcpy(y.data(), dy, count * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    double worst = 0.0;
    float at = 0.f;
    for (int i = 0; i < count; ++i) {
      const double t = which == 0 ? expm1((double)x[i]) : which == 1 ? log1p((double)x[i]) : exp((double)x[i]);
      const double e = fabs((double)y[i] - t) / ulp_of(t);
      if (e > worst) { worst = e; at = x[i]; }
    }
    printf("%s: worst error %.3f ulp at x = %.9g over %d arguments\n", names[which], worst, at, count);
  }
  return 0;
}
