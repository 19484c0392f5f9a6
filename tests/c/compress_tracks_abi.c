/* aclhip_compress_tracks_desc from a C99 translation unit: prints the struct's size and offsets for
 * tests/test_compress_tracks_arguments.py, compiles INTEGRATION.md's call sequence and makes calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

/* the call sequence INTEGRATION.md shows ("Transforms, with drop-w rotations") */
static aclhip_status integration_sequence(aclhip_context* gpu, const aclhip_raw_tracks* d_raws, uint32_t num_instances, uint32_t num_tracks, uint32_t max_tracks,
	const void* d_bind_pose, const uint32_t* d_parents, void* d_workspace, void* d_blobs, uint64_t stride, aclhip_compress_result* d_results, void* hip_stream)
{
	aclhip_compress_tracks_desc desc;
	memset(&desc, 0, sizeof(desc));
	desc.rotation_format = 2;
	desc.flags = ACLHIP_COMPRESS_OPTIMIZE_LOOPS | ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES;
	desc.default_pose = d_bind_pose;
	desc.parent_indices = d_parents;
	desc.num_table_tracks = num_tracks;
	desc.precision = 0.0001f; desc.shell_distance = 1.0f;
	desc.max_tracks = max_tracks;
	desc.workspace = d_workspace;
	desc.shell_metadata = NULL;
	return aclhip_compress_tracks_batch(gpu, d_raws, num_instances, &desc, d_blobs, stride, d_results, (void*)hip_stream);
}

int main(void)
{
	aclhip_compress_tracks_desc desc;
	uint32_t handles[4] = { 1, 1, 1, 1 };
	memset(&desc, 0, sizeof(desc));
	printf("%u\n", (unsigned)sizeof(aclhip_compress_tracks_desc));
	printf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %u\n", (unsigned)offsetof(aclhip_compress_tracks_desc, rotation_format),
		(unsigned)offsetof(aclhip_compress_tracks_desc, translation_format), (unsigned)offsetof(aclhip_compress_tracks_desc, scale_format),
		(unsigned)offsetof(aclhip_compress_tracks_desc, flags), (unsigned)offsetof(aclhip_compress_tracks_desc, max_tracks),
		(unsigned)offsetof(aclhip_compress_tracks_desc, num_table_tracks), (unsigned)offsetof(aclhip_compress_tracks_desc, default_pose),
		(unsigned)offsetof(aclhip_compress_tracks_desc, parent_indices), (unsigned)offsetof(aclhip_compress_tracks_desc, track_precisions),
		(unsigned)offsetof(aclhip_compress_tracks_desc, track_shell_distances), (unsigned)offsetof(aclhip_compress_tracks_desc, precision),
		(unsigned)offsetof(aclhip_compress_tracks_desc, shell_distance), (unsigned)offsetof(aclhip_compress_tracks_desc, workspace),
		(unsigned)offsetof(aclhip_compress_tracks_desc, shell_metadata), (unsigned)offsetof(aclhip_compress_tracks_desc, reserved));

	if (aclhip_compress_tracks_workspace_bytes(0, 100) != 0 || aclhip_compress_tracks_workspace_bytes(1, 1) != 64 + 16 + 16 + 16)
		return 1;
	if (aclhip_compress_tracks_batch(NULL, handles, 4, NULL, handles, 16, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	if (aclhip_compress_tracks_batch(NULL, handles, 4, &desc, NULL, 16, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 3;
	/* a sequence whose arguments pass every check ends at the missing context */
	if (integration_sequence(NULL, handles, 4, 4, 4, NULL, NULL, (void*)0x800000, (void*)0x100000, 4096, (aclhip_compress_result*)0x20000, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 4;
	return 0;
}
