// pcx_bary_seed2.hip -- the row-code MFMA kernels and launch tables for plans with R = 2 seed columns
// (BaryMfmaPlan::R; bary_mfma_launch.h), a translation unit of their own so that the sets compile side by side.

#include "bary_mfma_launch.h"

PCX_DEFINE_SEED_LAUNCHERS(2)
