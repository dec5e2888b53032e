/* Host build of the channel IQ's float -> 16-bit conversion (FMD_CIQ_S16): fmd_f32_to_mpx16 of csrc/fmd_math.h -- the
 * GPU executes the same source -- applied to both parts of a complex sample and packed as k_ciq_out packs them (re in
 * the low half of a 32-bit word, im in the high half, host byte order).  Reads complex float32 samples from the file
 * argv[1] and writes one packed word per sample to the file argv[2]; tests/test_ciq_cabi_cpu.py compares them with
 * the contract's numpy function mpx16() of the real and imaginary parts. */
#include <stdint.h>
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
  float x[2 * 4096];
  uint32_t y[4096];
  size_t n;
  while ((n = fread(x, 2 * sizeof(float), 4096, in)) > 0)
  {
    for (size_t i = 0; i < n; i++)
    {
      const unsigned re = (unsigned)fmd_f32_to_mpx16(x[2 * i]) & 0xffffu;
      const unsigned im = (unsigned)fmd_f32_to_mpx16(x[2 * i + 1]) & 0xffffu;
      y[i] = re | (im << 16);
    }
    if (fwrite(y, sizeof(uint32_t), n, out) != n)
      return 2;
  }
  fclose(in);
  fclose(out);
  return 0;
}
