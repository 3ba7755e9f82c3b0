// pcx_slider_internal.h -- the slider handle as the translation units that serve it see it (pcx_spline.hip creates and
// evaluates it, pcx_calculus.hip and pcx_slider_box.hip run its calculus and box integrals).  Not part of the ABI.
#pragma once

#include "pcx_bary_internal.h"
#include "gather_kernels.h"

// ---------------------------------------------------------------------------------
// slider handle (reference slider.py:80-341): slides are borrowed pcx_bary handles
// ---------------------------------------------------------------------------------
struct pcx_slider {
    int device = 0;
    hipStream_t stream = nullptr;
    int d = 0;
    double pivot = 0.0;
    std::vector<pcx_bary *> slides;      // borrowed
    std::vector<SliderCols> cols;        // the point columns slide s reads
    std::vector<int> owner;              // dimension -> slide
    int max_cols = 1;
    std::mutex mu;
    HostStage stage;                     // host-pointer batches
    Scratch s_cols, s_vals, s_partial;
    // tensor-product grids (pcx_piecewise_grid.hip): the slides' own grids one behind the other in s_grid, the sum
    // kernel's table in s_gridtab (uploaded from grid_tab_host), a host result in s_gridout; grid_done as in pcx_spline
    Scratch s_grid, s_gridtab, s_gridout;
    std::vector<long> grid_tab_host;
    hipEvent_t grid_done = nullptr;
    // ladders (pcx_piecewise_ladder.hip): shared xs, a one-dimensional owner's shared ladder
    Scratch s_ladder[2];
};

// Columns of the (d - 1)-wide fixed rows (every dimension but `dim`, increasing) that hold the dimensions `dims[0 .. nc)`.
static SliderCols slider_fixed_cols(const int *dims, int nc, int dim) {
    SliderCols c;
    c.nc = nc;
    for (int k = 0; k < PCX_MAX_DIMS; ++k) c.col[k] = 0;
    for (int k = 0; k < nc; ++k) c.col[k] = dims[k] < dim ? dims[k] : dims[k] - 1;
    return c;
}
