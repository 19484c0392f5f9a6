/* aclhip_compress_tracks_additive_batch, aclhip_compress_tracks_variable_additive_batch and aclhip_find_bit_rates_additive_batch from a
 * C99 translation unit, for tests/test_additive_compress_arguments.py: compiles INTEGRATION.md's call sequence and makes calls that
 * return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

/* the call sequence INTEGRATION.md shows ("Additive clips, compressed against their base") */
static aclhip_status integration_sequence(aclhip_context* gpu, const aclhip_raw_tracks* d_raws, const aclhip_raw_tracks* d_base_raws, uint32_t num_instances,
	uint32_t num_tracks, uint32_t max_tracks, uint32_t max_samples, const uint32_t* d_parents, uint8_t* d_bit_rates, void* d_blobs, uint64_t blob_stride,
	void* d_workspace, aclhip_compress_result* d_results, void* hip_stream)
{
	const uint64_t segment_stride = 4u * (uint64_t)max_tracks;
	const uint64_t instance_stride = segment_stride * aclhip_variable_compress_num_segments(max_samples);
	aclhip_additive_base base;
	aclhip_find_bit_rates_desc search;
	aclhip_compress_variable_desc compress;
	aclhip_status status;
	memset(&base, 0, sizeof(base));
	base.base_raws = d_base_raws;
	base.additive_format = ACLHIP_ADDITIVE_ADDITIVE1;
	memset(&search, 0, sizeof(search));
	search.flags = ACLHIP_COMPRESS_OPTIMIZE_LOOPS;
	search.parent_indices = d_parents;
	search.num_table_tracks = num_tracks;
	search.precision = 0.0001f; search.shell_distance = 1.0f;
	search.max_tracks = max_tracks;
	search.max_samples = max_samples;
	search.level = ACLHIP_LEVEL_AUTOMATIC;
	search.workspace = d_workspace;
	status = aclhip_find_bit_rates_additive_batch(gpu, d_raws, num_instances, &search, d_bit_rates, instance_stride, segment_stride, d_results, &base, hip_stream);
	if (status != ACLHIP_OK)
		return status;
	memset(&compress, 0, sizeof(compress));
	compress.flags = search.flags;
	compress.parent_indices = d_parents;
	compress.num_table_tracks = num_tracks;
	compress.precision = search.precision; compress.shell_distance = search.shell_distance;
	compress.max_tracks = max_tracks;
	compress.max_samples = max_samples;
	compress.bit_rates = d_bit_rates;
	compress.bit_rate_instance_stride = instance_stride;
	compress.bit_rate_segment_stride = segment_stride;
	compress.workspace = d_workspace;
	return aclhip_compress_tracks_variable_additive_batch(gpu, d_raws, num_instances, &compress, d_blobs, blob_stride, d_results, &base, hip_stream);
}

int main(void)
{
	aclhip_additive_base base;
	aclhip_compress_tracks_desc desc;
	uint32_t handles[4] = { 1, 1, 1, 1 };
	memset(&base, 0, sizeof(base));
	memset(&desc, 0, sizeof(desc));
	printf("%u %u\n", (unsigned)sizeof(aclhip_additive_base), (unsigned)offsetof(aclhip_additive_base, reserved));

	if (sizeof(aclhip_additive_base) != 32 || offsetof(aclhip_additive_base, additive_format) != 8 || offsetof(aclhip_additive_base, reserved) != 16)
		return 1;
	/* a NULL additive base is refused before anything else is looked at */
	if (aclhip_compress_tracks_additive_batch(NULL, handles, 4, &desc, (void*)0x100000, 4096, (aclhip_compress_result*)0x20000, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	if (strcmp(aclhip_last_error_message(NULL), "null additive base") != 0)
		return 3;
	base.additive_format = 4;
	if (aclhip_compress_tracks_variable_additive_batch(NULL, handles, 4, NULL, (void*)0x100000, 4096, NULL, &base, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 4;
	if (strcmp(aclhip_last_error_message(NULL), "unknown additive format 4") != 0)
		return 5;
	/* a sequence whose arguments pass every check ends at the missing context */
	if (integration_sequence(NULL, handles, (const aclhip_raw_tracks*)0x40000, 4, 4, 4, 100, NULL, (uint8_t*)0x30000, (void*)0x100000, 4096, (void*)0x800000,
			(aclhip_compress_result*)0x20000, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 6;
	if (strcmp(aclhip_last_error_message(NULL), "null context") != 0)
		return 7;
	return 0;
}
