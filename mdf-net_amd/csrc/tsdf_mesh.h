// Constants of tsdf_mesh.hip that the C ABI documents (include/mdfnet_hip.h: MDF_TSDF_*, MDF_MESH_WORKSPACE_BYTES).
#pragma once
#include "mdfnet_hip.h"

namespace mdf {
namespace tsdf {

constexpr int kChunk = MDF_TSDF_CHUNK;            // views per launch: their camera rows and map pointers travel in the kernel argument
constexpr int kCamFloats = MDF_TSDF_CAM_FLOATS;   // floats per view in the HOST camera table
constexpr int kR = 0, kT = 9, kFx = 12, kFy = 13, kCx = 14, kCy = 15, kDmax = 16;   // R row-major, t, intrinsics, largest valid depth
constexpr int kMeshPer = 4, kMeshChunk = 256 * kMeshPer;   // lattice points per thread and per block of mesh_scan_kernel
static_assert(kMeshChunk == MDF_MESH_CHUNK, "MDF_MESH_WORKSPACE_BYTES counts chunks of MDF_MESH_CHUNK points");
static_assert(kChunk <= 32, "a block's skipped views are one 32-bit mask");

}  // namespace tsdf
}  // namespace mdf
