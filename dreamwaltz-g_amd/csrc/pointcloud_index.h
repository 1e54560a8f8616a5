// pointcloud_index.h -- the reference's lattice order (include/dwg_pointcloud.h), shared by nerf_field.hip (lattice density) and
// pointcloud.hip (lattice points): one function from a flat index to (ix, iy, iz).
#pragma once
#include <stdint.h>

struct PcLattice {
    uint32_t nx, ny, nz;
    uint32_t sx, sy, sz;        // chunk length per axis: min(split, axis length)
};

// nx ny nz >= 1 and < 2^32 (so every product below fits 32 bits), split >= 1
static inline PcLattice pc_lattice(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t split) {
    PcLattice l;
    l.nx = nx; l.ny = ny; l.nz = nz;
    l.sx = split < nx ? split : nx; l.sy = split < ny ? split : ny; l.sz = split < nz ? split : nz;
    return l;
}

#if defined(__HIPCC__)
// Chunks (xi, yi, zi), zi fastest; inside a chunk (lx, ly, lz), lz fastest.  f < nx ny nz.
__device__ __forceinline__ void pc_lattice_decode(const PcLattice& l, uint32_t f, uint32_t& ix, uint32_t& iy, uint32_t& iz) {
    const uint32_t slab = l.sx * l.ny * l.nz;                   // points of one full x-chunk
    const uint32_t xi = f / slab;
    f -= xi * slab;
    const uint32_t cx = min(l.sx, l.nx - xi * l.sx);
    const uint32_t row = cx * l.sy * l.nz;                      // points of one full y-chunk inside this x-chunk
    const uint32_t yi = f / row;
    f -= yi * row;
    const uint32_t cy = min(l.sy, l.ny - yi * l.sy);
    const uint32_t cell = cx * cy * l.sz;                       // points of one full z-chunk inside this (x, y)-chunk
    const uint32_t zi = f / cell;
    f -= zi * cell;
    const uint32_t cz = min(l.sz, l.nz - zi * l.sz);
    const uint32_t lx = f / (cy * cz);
    f -= lx * cy * cz;
    const uint32_t ly = f / cz;
    ix = xi * l.sx + lx;
    iy = yi * l.sy + ly;
    iz = zi * l.sz + (f - ly * cz);
}
#endif
