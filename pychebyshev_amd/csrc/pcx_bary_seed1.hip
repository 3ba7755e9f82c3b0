// pcx_bary_seed1.hip -- the row-code MFMA kernels and launch tables for plans with R = 1 seed column
// (BaryMfmaPlan::R; bary_mfma_launch.h), a translation unit of their own so that the sets compile side by side.

#include "bary_mfma_launch.h"

PCX_DEFINE_SEED_LAUNCHERS(1)
