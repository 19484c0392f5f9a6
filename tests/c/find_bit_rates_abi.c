/* aclhip_find_bit_rates_desc from a C99 translation unit: prints the struct's size and offsets for
 * tests/test_bit_rate_search_arguments.py, compiles INTEGRATION.md's call sequence and makes calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

/* the call sequence INTEGRATION.md shows ("Transforms, in the variable formats at the rates the search finds") */
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
	search.level = 2;
	search.workspace = d_workspace;
	return aclhip_find_bit_rates_batch(gpu, d_raws, num_instances, &search, d_bit_rates, instance_stride, segment_stride, d_results, (void*)hip_stream);
}

int main(void)
{
	aclhip_find_bit_rates_desc desc;
	uint32_t handles[4] = { 1, 1, 1, 1 };
	memset(&desc, 0, sizeof(desc));
	printf("%u\n", (unsigned)sizeof(aclhip_find_bit_rates_desc));
	printf("%u %u %u %u %u %u %u %u ", (unsigned)offsetof(aclhip_find_bit_rates_desc, flags), (unsigned)offsetof(aclhip_find_bit_rates_desc, max_tracks),
		(unsigned)offsetof(aclhip_find_bit_rates_desc, max_samples), (unsigned)offsetof(aclhip_find_bit_rates_desc, num_table_tracks),
		(unsigned)offsetof(aclhip_find_bit_rates_desc, default_pose), (unsigned)offsetof(aclhip_find_bit_rates_desc, parent_indices),
		(unsigned)offsetof(aclhip_find_bit_rates_desc, track_precisions), (unsigned)offsetof(aclhip_find_bit_rates_desc, track_shell_distances));
	printf("%u %u %u %u %u %u %u\n", (unsigned)offsetof(aclhip_find_bit_rates_desc, precision), (unsigned)offsetof(aclhip_find_bit_rates_desc, shell_distance),
		(unsigned)offsetof(aclhip_find_bit_rates_desc, workspace), (unsigned)offsetof(aclhip_find_bit_rates_desc, shell_metadata),
		(unsigned)offsetof(aclhip_find_bit_rates_desc, level), (unsigned)offsetof(aclhip_find_bit_rates_desc, reserved_word),
		(unsigned)offsetof(aclhip_find_bit_rates_desc, reserved));

	if (aclhip_find_bit_rates_workspace_bytes(0, 100, 100) != 0 || aclhip_find_bit_rates_workspace_bytes(1, 1, 1) % 16 != 0)
		return 1;
	if (aclhip_find_bit_rates_batch(NULL, handles, 4, NULL, (uint8_t*)0x30000, 64, 16, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	if (aclhip_find_bit_rates_batch(NULL, handles, 4, &desc, NULL, 64, 16, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 3;
	/* a sequence whose arguments pass every check ends at the missing context */
	if (integration_sequence(NULL, handles, 4, 4, 4, 100, NULL, NULL, (uint8_t*)0x30000, (void*)0x800000, (aclhip_compress_result*)0x20000, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 4;
	return 0;
}
