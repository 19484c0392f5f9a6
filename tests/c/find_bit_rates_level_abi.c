/* aclhip_find_bit_rates_level_batch from a C99 translation unit, for tests/test_bit_rate_search_levels_arguments.py: compiles
 * INTEGRATION.md's call sequence and makes calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

/* the call sequence INTEGRATION.md shows ("Transforms, in the variable formats at the reference's default level") */
static aclhip_status integration_sequence(aclhip_context* gpu, const aclhip_raw_tracks* d_raws, uint32_t num_instances, uint32_t num_tracks, uint32_t max_tracks,
	uint32_t max_samples, const void* d_bind_pose, const uint32_t* d_parents, uint8_t* d_bit_rates, void* d_workspace, aclhip_compress_result* d_results, void* hip_stream)
{
	const uint64_t segment_stride = 4u * (uint64_t)max_tracks;
	const uint64_t instance_stride = segment_stride * aclhip_variable_compress_num_segments(max_samples);
	aclhip_find_bit_rates_desc search;
	memset(&search, 0, sizeof(search));
	search.flags = ACLHIP_COMPRESS_OPTIMIZE_LOOPS;
	search.default_pose = d_bind_pose;
	search.parent_indices = d_parents;
	search.num_table_tracks = num_tracks;
	search.precision = 0.0001f; search.shell_distance = 1.0f;
	search.max_tracks = max_tracks;
	search.max_samples = max_samples;
	search.level = ACLHIP_LEVEL_AUTOMATIC;
	search.workspace = d_workspace;
	return aclhip_find_bit_rates_level_batch(gpu, d_raws, num_instances, &search, d_bit_rates, instance_stride, segment_stride, d_results, ACLHIP_METRIC_QVVF, (void*)hip_stream);
}

int main(void)
{
	aclhip_find_bit_rates_desc desc;
	uint32_t handles[4] = { 1, 1, 1, 1 };
	memset(&desc, 0, sizeof(desc));
	printf("%u\n", (unsigned)ACLHIP_LEVEL_AUTOMATIC);

	if (aclhip_find_bit_rates_level_workspace_bytes(0, 100, 100) != 0 || aclhip_find_bit_rates_level_workspace_bytes(1, 1, 1) % 16 != 0)
		return 1;
	if (aclhip_find_bit_rates_level_workspace_bytes(3, 65, 65) < aclhip_find_bit_rates_workspace_bytes(3, 65, 65))
		return 2;
	if (aclhip_find_bit_rates_level_batch(NULL, handles, 4, NULL, (uint8_t*)0x30000, 64, 16, NULL, ACLHIP_METRIC_QVVF, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 3;
	if (aclhip_find_bit_rates_level_batch(NULL, handles, 4, &desc, NULL, 64, 16, NULL, ACLHIP_METRIC_QVVF_MATRIX3X4F, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 4;
	/* a sequence whose arguments pass every check ends at the missing context */
	if (integration_sequence(NULL, handles, 4, 4, 4, 100, NULL, NULL, (uint8_t*)0x30000, (void*)0x800000, (aclhip_compress_result*)0x20000, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 5;
	if (strcmp(aclhip_last_error_message(NULL), "null context") != 0)
		return 6;
	return 0;
}
