/* aclhip_compress_variable_desc from a C99 translation unit: prints the struct's size and offsets for
 * tests/test_variable_compress_arguments.py, compiles INTEGRATION.md's call sequence and makes calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

/* the call sequence INTEGRATION.md shows ("Transforms, in the variable formats at given bit rates") */
static aclhip_status integration_sequence(aclhip_context* gpu, const aclhip_raw_tracks* d_raws, uint32_t num_instances, uint32_t num_tracks, uint32_t max_tracks,
	uint32_t max_samples, const void* d_bind_pose, const uint32_t* d_parents, const uint8_t* d_bit_rates, void* d_workspace, void* d_blobs, uint64_t stride,
	aclhip_compress_result* d_results, void* hip_stream)
{
	aclhip_compress_variable_desc desc;
	memset(&desc, 0, sizeof(desc));
	desc.flags = ACLHIP_COMPRESS_OPTIMIZE_LOOPS | ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES;
	desc.default_pose = d_bind_pose;
	desc.parent_indices = d_parents;
	desc.num_table_tracks = num_tracks;
	desc.precision = 0.0001f; desc.shell_distance = 1.0f;
	desc.max_tracks = max_tracks;
	desc.max_samples = max_samples;
	desc.bit_rates = d_bit_rates;
	desc.bit_rate_segment_stride = 4u * max_tracks;
	desc.bit_rate_instance_stride = desc.bit_rate_segment_stride * aclhip_variable_compress_num_segments(max_samples);
	desc.rotation_bit_rate = 16; desc.translation_bit_rate = 16; desc.scale_bit_rate = 16;
	desc.workspace = d_workspace;
	return aclhip_compress_tracks_variable_batch(gpu, d_raws, num_instances, &desc, d_blobs, stride, d_results, (void*)hip_stream);
}

int main(void)
{
	aclhip_compress_variable_desc desc;
	uint32_t handles[4] = { 1, 1, 1, 1 };
	memset(&desc, 0, sizeof(desc));
	printf("%u\n", (unsigned)sizeof(aclhip_compress_variable_desc));
	printf("%u %u %u %u %u %u %u %u ", (unsigned)offsetof(aclhip_compress_variable_desc, flags), (unsigned)offsetof(aclhip_compress_variable_desc, max_tracks),
		(unsigned)offsetof(aclhip_compress_variable_desc, max_samples), (unsigned)offsetof(aclhip_compress_variable_desc, num_table_tracks),
		(unsigned)offsetof(aclhip_compress_variable_desc, default_pose), (unsigned)offsetof(aclhip_compress_variable_desc, parent_indices),
		(unsigned)offsetof(aclhip_compress_variable_desc, track_precisions), (unsigned)offsetof(aclhip_compress_variable_desc, track_shell_distances));
	printf("%u %u %u %u %u %u %u ", (unsigned)offsetof(aclhip_compress_variable_desc, precision), (unsigned)offsetof(aclhip_compress_variable_desc, shell_distance),
		(unsigned)offsetof(aclhip_compress_variable_desc, workspace), (unsigned)offsetof(aclhip_compress_variable_desc, shell_metadata),
		(unsigned)offsetof(aclhip_compress_variable_desc, bit_rates), (unsigned)offsetof(aclhip_compress_variable_desc, bit_rate_instance_stride),
		(unsigned)offsetof(aclhip_compress_variable_desc, bit_rate_segment_stride));
	printf("%u %u %u %u %u %u\n", (unsigned)offsetof(aclhip_compress_variable_desc, rotation_bit_rate), (unsigned)offsetof(aclhip_compress_variable_desc, translation_bit_rate),
		(unsigned)offsetof(aclhip_compress_variable_desc, scale_bit_rate), (unsigned)offsetof(aclhip_compress_variable_desc, reserved_rate),
		(unsigned)offsetof(aclhip_compress_variable_desc, reserved_word), (unsigned)offsetof(aclhip_compress_variable_desc, reserved));

	if (aclhip_variable_compress_num_segments(31) != 1 || aclhip_variable_compress_num_segments(32) != 2 || aclhip_variable_compress_num_segments(33) != 2
		|| aclhip_variable_compress_num_segments(49) != 3)
		return 1;
	if (aclhip_compress_variable_workspace_bytes(0, 100, 100) != 0 || aclhip_variable_compress_bound(1, 1, 0) % 16 != 0 || aclhip_variable_compress_bound(1, 1, 0) < 151)
		return 2;
	if (aclhip_compress_tracks_variable_batch(NULL, handles, 4, NULL, handles, 16, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 3;
	if (aclhip_compress_tracks_variable_batch(NULL, handles, 4, &desc, NULL, 16, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 4;
	/* a sequence whose arguments pass every check ends at the missing context */
	if (integration_sequence(NULL, handles, 4, 4, 4, 100, NULL, NULL, (const uint8_t*)0x30000, (void*)0x800000, (void*)0x100000, 4096, (aclhip_compress_result*)0x20000, NULL)
		!= ACLHIP_ERROR_INVALID_ARGUMENT)
		return 5;
	return 0;
}
