// pt_volume.hip — the kernel of pt_update_volumes (gfx950): a Volume's derived tables rebuilt on the device from new
// voxels or new windows.  The per-cell rules are pt_volume_update.h's, shared with the upload's host
// loops.
//   k_vol_cells_runs  one lane per cell of the (w+1)(h+1)(d+1) lattice, x fastest, blocks of 256 lanes, a grid-stride
//                     loop over at most kVolMaxBlocks blocks.  A cell takes its eight corners, writes its 64-B
//                     cell-major record (kWriteCells) and its sign byte.
// Three instantiations of one kernel text:
//   new voxels, a volume with cells     corners from the voxel array by the vol_get rule (zeros outside the grid);
//                                        record and sign written.  Neighbouring lanes are neighbouring x, so the eight
//                                        reads of a wave fall on four pairs of voxel rows: every line is read by the
//                                        lanes that share it, and the 8x re-read of a voxel is served by L2.
//   new voxels, a volume without cells  the same, no record stores.
//   new windows only, with cells        corners from the cell's own record, one half-line per cell (four 16-B loads)
//                                        instead of eight scattered reads; only the sign written.  Without cells a
//                                        windows-only update runs the second form.
// Stores: a record is four 16-B vector stores per lane, a wave covering 4 KiB contiguous.  The sign is one byte store
// per lane, a wave covering 64 contiguous bytes.  Packing four cells' signs into one 32-bit store (lanes 4k..4k+3
// gathered by shuffles, the table's unaligned first and last words written byte by byte: a volume's table starts at
// the sum of the earlier volumes' cell counts) was built and measured on the 256x256x128 Volume of
// tools/volume_update_bench.py: 0.2718 ms against 0.2737 ms with new voxels, 0.1404 against 0.1406 ms with new windows
// only, inside each other's min-max ranges.  The signs are 1/64 of the bytes the kernel moves; the byte stores stay.
// Every index and byte offset is 64-bit.  Plain vector stores only, one writer per word; launches on one
// stream are ordered; no atomics.  A lane outside the table loads and stores nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_volume_update.h"

#pragma clang fp contract(off)

namespace pt {

constexpr int kVolBlock = 256;
constexpr uint64_t kVolMaxBlocks = 4096;

template <bool kFromCells, bool kWriteCells>
__global__ __launch_bounds__(kVolBlock) void k_vol_cells_runs(DevVolume v, double* __restrict__ cells, int8_t* __restrict__ runs,
                                                              uint64_t ncells) {
    for (uint64_t i = (uint64_t)blockIdx.x * kVolBlock + threadIdx.x; i < ncells; i += (uint64_t)gridDim.x * kVolBlock) {
        double c[8];
        if (kFromCells) {
            PT_GLOBAL(VolPair) p = (PT_GLOBAL(VolPair))(v.cells + vol_cell_first(i));
            const VolPair a = p[0], b = p[1], e = p[2], f = p[3];
            c[0] = a.lo; c[1] = a.hi; c[2] = b.lo; c[3] = b.hi; c[4] = e.lo; c[5] = e.hi; c[6] = f.lo; c[7] = f.hi;
        } else {
            int x0, y0, z0;
            vol_cell_coords(v.w, v.h, i, x0, y0, z0);
            vol_cell_corners(v, x0, y0, z0, c);
        }
        if (kWriteCells) {
            VolPair* q = (VolPair*)(cells + vol_cell_first(i));
            q[0] = VolPair{c[0], c[1]};
            q[1] = VolPair{c[2], c[3]};
            q[2] = VolPair{c[4], c[5]};
            q[3] = VolPair{c[6], c[7]};
        }
        runs[i] = vol_cell_sign(v, c);
    }
}

// Volume v's tables rebuilt on `stream`; v holds device addresses (data, windows, runs, cells; cells NULL: the volume has
// none).  new_data: the voxels changed (corners from them, the records rewritten); else only the windows did.
hipError_t launch_vol_rebuild(const DevVolume& v, bool new_data, hipStream_t stream) {
    const uint64_t ncells = vol_cell_count(v.w, v.h, v.d);
    if (!v.runs) return hipSuccess;
    const uint64_t blocks = (ncells + kVolBlock - 1) / kVolBlock;
    const dim3 grid((unsigned)(blocks < kVolMaxBlocks ? blocks : kVolMaxBlocks)), block(kVolBlock);
    double* cells = const_cast<double*>(v.cells);
    int8_t* runs = const_cast<int8_t*>(v.runs);
    const int form = (new_data && cells) ? 0 : (!new_data && cells) ? 2 : 1;
#define PT_VOL_LAUNCH(FROM, WRITE) \
    hipLaunchKernelGGL((k_vol_cells_runs<FROM, WRITE>), grid, block, 0, stream, v, cells, runs, ncells)
    if (form == 0) PT_VOL_LAUNCH(false, true);
    else if (form == 2) PT_VOL_LAUNCH(true, false);
    else PT_VOL_LAUNCH(false, false);
#undef PT_VOL_LAUNCH
    return hipGetLastError();
}

}  // namespace pt
