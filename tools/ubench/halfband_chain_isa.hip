// The half-band chain's kernels (k_halfband_chain, all four forms) as a compile unit of their own: what
// tools/isa_chain_table.py compiles to count the step loop's instructions.  Not a program: no main.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -S --cuda-device-only \
//         -I pvr.rtl.radiofm_amd/csrc tools/ubench/halfband_chain_isa.hip -o chain.s
#include <hip/hip_runtime.h>

#include "fmd_k_rds.hip.h"

// taking a kernel's address instantiates it, whatever its parameter list is
void* const fmd_chain_forms[] = {
    (void*)&fmd::k_halfband_chain<7, 11, 21, true>, (void*)&fmd::k_halfband_chain<7, 11, 21, false>,
    (void*)&fmd::k_halfband_chain<7, 9, 17, true>, (void*)&fmd::k_halfband_chain<7, 9, 17, false>};
