// grid.h -- the uniform-grid binning of a point set that knn.hip builds (bounding box, per-cell counts, scan, scatter), shared with
// align.hip.  The kernels live in knn.hip; these are its two host steps.
#pragma once
#include "common.h"

// cell (i, j) covers [x0 + i / inv_cell, x0 + (i+1) / inv_cell) x [y0 + j / inv_cell, ...), row-major, gx x gy cells
struct GridDesc {
    double x0, y0, inv_cell;
    int gx, gy;
};

// the cell coordinate a point is binned under: floor((v - v0) * inv_cell) clamped to [0, g)
__device__ __forceinline__ int cell_coord(double v, double v0, double inv_cell, int g) {
    const double c = __builtin_floor((v - v0) * inv_cell);
    return c < 0.0 ? 0 : (c >= (double)g ? g - 1 : (int)c);
}

// box = {min x, min y, max x, max y} of dxy[0, n) (n >= 1): a device reduction and one 32-byte read-back, synchronous
int grid_bbox(same_ctx *ctx, const double *dxy, int64_t n, double box[4]);
// counting sort of dxy[0, n) (n >= 1) by cell, enqueue only: dstart[cells + 1] (exclusive scan of the counts), the sorted XY dsxy[n][2]
// and the original index of each sorted point dsidx[n]; drank[n] is scratch
int grid_fill(same_ctx *ctx, const double *dxy, int64_t n, const GridDesc &g, unsigned *dstart, unsigned *drank, double *dsxy,
              int32_t *dsidx);
