/* Host build of the signed integer IQ conversions of csrc/fmd_math.h (the GPU executes the same source): prints the
 * float bits of every int16 value (65 536 lines "s16 <value> <bits>") and of every int8 value (256 lines "s8 ...").
 * tests/test_iq_formats_cabi_cpu.py compares them with numpy's v.astype(float32) * float32(2**-15 | 2**-7). */
#include <stdio.h>

#include "fmd_math.h"

int main(void)
{
  for (int v = -32768; v <= 32767; v++)
    printf("s16 %d %08x\n", v, (unsigned)fmd_f2u(fmd_s16_to_f32((int16_t)v)));
  for (int v = -128; v <= 127; v++)
    printf("s8 %d %08x\n", v, (unsigned)fmd_f2u(fmd_s8_to_f32((int8_t)v)));
  return 0;
}
