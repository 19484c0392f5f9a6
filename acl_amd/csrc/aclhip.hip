// aclhip.hip -- gfx950 decode kernels and the host side of the C ABI of libaclhip.so (include/aclhip.h).
//
// One translation unit, in parts: the kernels live in kernels_*.inl, the host side in host_*.inl, included at the end of this file.
//
// Kernels (device helpers in aclhip_device.h):
//   decompress_tracks_kernel / decompress_tracks_any_settings_kernel
//       one wave64 per (clip instance, window of 312 pose quads = 104 tracks): scalar seek, base pose DMA'd global -> LDS, lanes <-> animated
//       sub-tracks decode in place into the LDS image (bit unpack, segment + clip range, W, lerp, normalize), the window streams
//       out 1 KiB per store instruction. The second entry point is the same body with per track rounding, the non default
//       default sub-track modes and always-normalize compiled in. Poses of several windows: decompress_tracks_in_turn_kernel (a wave
//       takes four work items in turn and keeps its LDS image while the clip stays the same; one 16 byte read of the bitstream per key).
//       Every launch is shaped by its batch (pose stride) and every kernel checks the clips it meets against that shape.
//   decompress_poses_consumer_kernel   the same decode, whole pose per wave, followed by what callers do next with a local pose -- blend K
//                                      clip instances, apply an additive clip onto its base, local -> object space -- before the pose leaves LDS.
//   transform_poses_kernel             the same consumers over a caller's pose buffers: the LDS image is filled from a row in HBM, not from a clip.
//   sample_raw_tracks_kernel           uncompressed clips (raw track arrays): one lane per quad of the pose row, two 16 byte loads, one store.
//   sample_raw_scalar_tracks_kernel    uncompressed scalar curve sets (raw scalar track arrays): one lane per float of the value row (four floats where row and key frames are 16 byte aligned), two loads, one store.
//   sample_raw_scalar_track_kernel     the same arrays, one thread per (instance, track) request.
//   measure_scalar_error_kernel        the scalar track error of two value buffers: one wave64 per instance, lanes <-> tracks.
//   scalar_compress_*_kernel           compress_track_list of raw scalar track arrays in five launches: vote, per-track analysis (one wave64 per track), layout, bit stream (one lane per output dword), hash (compress_hash_kernel, the transform compressor's too).
//   tracks_compress_*_kernel           compress_track_list with drop-w rotations: the rigid shell and the looping vote (one wave64 per instance), the shell error analysis (one wave64 per track), then the raw-format compressor's layout and stream with three words per rotation.
//   decompress_track_kernel            one thread per (instance, bone) request; the registration time plan replaces the
//                                      reference's O(track index) skip over preceding widths.
//   decompress_scalar_tracks_kernel    scalar track lists: one wave64 per (instance, 256 tracks), lanes <-> tracks.
//   decompress_scalar_track_kernel     scalar track lists: one thread per (instance, track) request.
//   apply_tier_metadata_kernel         publishes / retires database tier metadata behind a stream ordered bulk copy.
//
// Every output store is a streaming store (store_streaming, aclhip_device.h): poses must not evict clip data from the L2s.
//
// Host side: context and clip / database registries (clips live in shared HBM slabs), blob validation, registration time tables,
// walk schedules of hierarchies, locality order of instance lists, launches.
//
// Build (acl_amd/build.py): hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -mllvm -amdgpu-kernarg-preload-count=16 aclhip.hip -ldl -o ../lib/libaclhip.so
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <new>
#include <string>
#include <unordered_set>
#include <type_traits>
#include <vector>

#include "../../include/aclhip.h"
#include "acl_format.h"
#include "aclhip_device.h"

namespace aclhip
{
#include "kernels_pose.inl"
#if defined(ACLHIP_EXPERIMENTS)
#include "../../tools/experiments/kernels_experiments.inl"		// round 3's slower variants (profiles/r03_experiments.md); not part of a default build
#endif
#include "kernels_consumers.inl"
#include "kernels_skeleton.inl"
#include "kernels_pose_buffers.inl"
#include "kernels_raw_tracks.inl"
#include "kernels_raw_scalar_tracks.inl"
#include "kernels_scalar_compress.inl"
#include "kernels_transform_compress.inl"
#include "kernels_tracks_compress.inl"
#include "kernels_variable_compress.inl"
#include "kernels_bit_rate_search.inl"
#include "kernels_misc.inl"
#include "kernels_scalar.inl"
#include "kernels_track.inl"
#include "kernels_bone_object.inl"
}

// ================================================================================================
// Host side: context, clip registry, C ABI
// ================================================================================================
using namespace aclhip;

#include "host_context.inl"
#include "host_clips.inl"
#include "host_databases.inl"
#if defined(ACLHIP_EXPERIMENTS)
#include "../../tools/experiments/host_experiments.inl"
#endif
#include "host_launch.inl"
#include "host_track_maps.inl"
#include "host_lists.inl"
#include "host_consumers.inl"
#include "host_skeletons.inl"
#include "host_blend_masks.inl"
#include "host_ranges.inl"
#include "host_pose_buffers.inl"
#include "host_skins.inl"
#include "host_raw_tracks.inl"
#include "host_raw_scalar_tracks.inl"
#include "host_scalar_compress.inl"
#include "host_transform_compress.inl"
#include "host_bone_object.inl"
#include "host_scalar_misc.inl"
