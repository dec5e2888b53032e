/* Host build of the float -> 16-bit multiplex conversion of csrc/fmd_math.h (the GPU executes the same source):
 * reads float32 values from the file argv[1] and writes fmd_f32_to_mpx16 of each as int16 to the file argv[2].
 * tests/test_mpx_cabi_cpu.py compares them with the contract's numpy function mpx16().  The header's remark that
 * fmd_f32_to_s16(x * 0.25f) is the same integer for every float is held against the same values here. */
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
  size_t n;
  while ((n = fread(x, sizeof(float), 4096, in)) > 0)
  {
    for (size_t i = 0; i < n; i++)
    {
      const int v = fmd_f32_to_mpx16(x[i]);
      if (v < -32768 || v > 32767 || v != fmd_f32_to_s16(x[i] * 0.25f))
        return 3;
      y[i] = (int16_t)v;
    }
    if (fwrite(y, sizeof(int16_t), n, out) != n)
      return 2;
  }
  fclose(in);
  fclose(out);
  return 0;
}
