/* Host build of the float -> 16-bit PCM conversion of csrc/fmd_math.h (the GPU executes the same source):
 * reads float32 values from the file argv[1], writes fmd_f32_to_s16 of each as int16 to the file argv[2] and the
 * number of them fmd_f32_to_s16_count counted as clipped to stdout.  tests/test_pcm_formats_cabi_cpu.py compares
 * them with the contract's numpy function pcm16(). */
#include <stdio.h>
#include <stdlib.h>

#include "fmd_math.h"

int main(int argc, char** argv)
{
  if (argc != 3)
    return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out)
    return 2;
  float x[4096];
  int16_t y[4096];
  unsigned long long clipped = 0;
  size_t n;
  while ((n = fread(x, sizeof(float), 4096, in)) > 0)
  {
    for (size_t i = 0; i < n; i++)
    {
      unsigned c = 0;
      const int v = fmd_f32_to_s16_count(x[i], &c);
      if (v != fmd_f32_to_s16(x[i]) || v < -32768 || v > 32767)
        return 3;
      y[i] = (int16_t)v;
      clipped += c;
    }
    if (fwrite(y, sizeof(int16_t), n, out) != n)
      return 2;
  }
  fclose(in);
  fclose(out);
  printf("%llu\n", clipped);
  return 0;
}
