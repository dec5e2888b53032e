// The headline forms of the IF FIR (k_if_fir_mt3, two and three outputs per lane, float and byte input, with and
// without a capture map) as a compile unit of their own: what tools/isa_fir_table.py compiles to count what a tile
// issues.  Not a program: no main.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -S --cuda-device-only \
//         -I pvr.rtl.radiofm_amd/csrc tools/ubench/if_fir_isa.hip -o fir.s
#include <hip/hip_runtime.h>

#include <type_traits>

#include "fmd_k_if.hip.h"

// taking a kernel's address instantiates it, whatever its parameter list is
void* const fmd_fir_forms[] = {
    (void*)&fmd::k_if_fir_mt3<fmd::InF32, 12, 2, 2, 88, 11, false, false>,
    (void*)&fmd::k_if_fir_mt3<fmd::InU8, 12, 2, 2, 88, 11, false, false>,
    (void*)&fmd::k_if_fir_mt3<fmd::InS16, 12, 2, 2, 88, 11, false, false>,
    (void*)&fmd::k_if_fir_mt3<fmd::InF32, 12, 2, 2, 88, 11, false, true>,
    (void*)&fmd::k_if_fir_mt3<fmd::InF32, 18, 2, 3, 88, 11, false, false>};
