/* The three transform compressors with the error metric as an argument from a C99 translation unit, for
 * tests/test_matrix_metric_compress_arguments.py: their prototypes held to function pointer types spelled out here, and calls that
 * return before any device call. */
#include <stddef.h>
#include <string.h>

#include "aclhip.h"

typedef aclhip_status (*compress_tracks_metric_fn)(aclhip_context*, const aclhip_raw_tracks*, uint32_t, const aclhip_compress_tracks_desc*, void*, uint64_t,
	aclhip_compress_result*, uint32_t, void*);
typedef aclhip_status (*compress_variable_metric_fn)(aclhip_context*, const aclhip_raw_tracks*, uint32_t, const aclhip_compress_variable_desc*, void*, uint64_t,
	aclhip_compress_result*, uint32_t, void*);
typedef aclhip_status (*find_bit_rates_metric_fn)(aclhip_context*, const aclhip_raw_tracks*, uint32_t, const aclhip_find_bit_rates_desc*, uint8_t*, uint64_t, uint64_t,
	aclhip_compress_result*, uint32_t, void*);

int main(void)
{
	/* (an assignment between function pointer types that differ is a constraint violation: -pedantic -Werror stops the build) */
	const compress_tracks_metric_fn compress_tracks = aclhip_compress_tracks_metric_batch;
	const compress_variable_metric_fn compress_variable = aclhip_compress_tracks_variable_metric_batch;
	const find_bit_rates_metric_fn find_bit_rates = aclhip_find_bit_rates_metric_batch;
	uint32_t handles[4] = { 1, 1, 1, 1 };
	aclhip_compress_tracks_desc tracks;
	aclhip_compress_variable_desc variable;
	aclhip_find_bit_rates_desc search;
	uint32_t metric;
	memset(&tracks, 0, sizeof(tracks));
	memset(&variable, 0, sizeof(variable));
	memset(&search, 0, sizeof(search));
	tracks.rotation_format = 2;
	tracks.max_tracks = variable.max_tracks = search.max_tracks = 4;
	variable.max_samples = search.max_samples = 40;
	tracks.precision = variable.precision = search.precision = 0.0001f;
	tracks.shell_distance = variable.shell_distance = search.shell_distance = 1.0f;
	tracks.workspace = variable.workspace = search.workspace = (void*)0x800000;
	variable.rotation_bit_rate = variable.translation_bit_rate = variable.scale_bit_rate = 12;
	search.level = 2;

	/* both metrics pass every check and end at the missing context; a third is refused */
	for (metric = ACLHIP_METRIC_QVVF; metric <= ACLHIP_METRIC_QVVF_MATRIX3X4F + 1u; ++metric)
	{
		const char* expected = metric <= ACLHIP_METRIC_QVVF_MATRIX3X4F ? "null context" : "unknown error metric 2";
		if (compress_tracks(NULL, handles, 4, &tracks, (void*)0x100000, 4096, (aclhip_compress_result*)0x20000, metric, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT
			|| strcmp(aclhip_last_error_message(NULL), expected) != 0)
			return 1 + (int)metric;
		if (compress_variable(NULL, handles, 4, &variable, (void*)0x100000, 4096, (aclhip_compress_result*)0x20000, metric, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT
			|| strcmp(aclhip_last_error_message(NULL), expected) != 0)
			return 4 + (int)metric;
		if (find_bit_rates(NULL, handles, 4, &search, (uint8_t*)0x30000, 64, 16, (aclhip_compress_result*)0x20000, metric, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT
			|| strcmp(aclhip_last_error_message(NULL), expected) != 0)
			return 7 + (int)metric;
	}
	return 0;
}
