/* aclhip_raw_scalar_tracks_info and aclhip_scalar_error_desc from a C99 translation unit: prints the structs' sizes and offsets for
 * tests/test_raw_scalar_tracks_abi.py, and makes calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

int main(void)
{
	aclhip_scalar_error_desc desc;
	aclhip_raw_scalar_tracks_info info;
	aclhip_raw_scalar_tracks raw = 99;
	aclhip_track_error records[4];
	aclhip_track_error_worst worst;
	char message[128];
	float samples[24] = { 0.0f };
	uint32_t handles[4] = { 1, 1, 1, 1 };
	uint32_t tracks[4] = { 0, 0, 0, 0 };
	float times[4] = { 0.0f };
	float rows[48] = { 0.0f };
	memset(&desc, 0, sizeof(desc));
	memset(&worst, 0, sizeof(worst));
	printf("%u %u\n", (unsigned)sizeof(aclhip_scalar_error_desc), (unsigned)sizeof(aclhip_raw_scalar_tracks_info));
	printf("%u %u %u %u %u %u\n", (unsigned)offsetof(aclhip_scalar_error_desc, num_tracks), (unsigned)offsetof(aclhip_scalar_error_desc, num_components),
		(unsigned)offsetof(aclhip_scalar_error_desc, track_errors), (unsigned)offsetof(aclhip_scalar_error_desc, track_error_stride_bytes),
		(unsigned)offsetof(aclhip_scalar_error_desc, worst), (unsigned)offsetof(aclhip_scalar_error_desc, reserved));
	printf("%u %u %u %u %u %u %u %u\n", (unsigned)offsetof(aclhip_raw_scalar_tracks_info, num_tracks), (unsigned)offsetof(aclhip_raw_scalar_tracks_info, num_samples),
		(unsigned)offsetof(aclhip_raw_scalar_tracks_info, sample_rate), (unsigned)offsetof(aclhip_raw_scalar_tracks_info, duration),
		(unsigned)offsetof(aclhip_raw_scalar_tracks_info, looping_policy), (unsigned)offsetof(aclhip_raw_scalar_tracks_info, track_type),
		(unsigned)offsetof(aclhip_raw_scalar_tracks_info, num_components), (unsigned)offsetof(aclhip_raw_scalar_tracks_info, reserved));
	printf("%u %u %u %u %u\n", (unsigned)ACLHIP_MAX_RAW_SCALAR_TRACKS, (unsigned)sizeof(aclhip_raw_scalar_tracks), (unsigned)sizeof(aclhip_track_error),
		(unsigned)sizeof(aclhip_track_error_worst), (unsigned)(ACLHIP_NO_TRACK == 0xFFFFFFFFu));

	if (aclhip_check_raw_scalar_tracks(samples, 2, 4, 2, 30.0f, ACLHIP_LOOP_WRAP, &info, message, sizeof(message)) != ACLHIP_OK || info.num_samples != 2
		|| info.looping_policy != ACLHIP_LOOP_WRAP || info.track_type != 2 || info.num_components != 3)
		return 1;
	if (aclhip_check_raw_scalar_tracks(samples, 12, 1, 2, 30.0f, ACLHIP_LOOP_CLAMP, &info, message, sizeof(message)) != ACLHIP_ERROR_INVALID_ARGUMENT || strstr(message, "qvvf") == NULL)
		return 2;
	if (aclhip_register_raw_scalar_tracks(NULL, samples, 0, 1, 2, 30.0f, ACLHIP_LOOP_CLAMP, &raw) != ACLHIP_ERROR_INVALID_ARGUMENT || raw != 0)
		return 3;
	if (aclhip_unregister_raw_scalar_tracks(NULL, 1) != ACLHIP_ERROR_INVALID_ARGUMENT || aclhip_get_raw_scalar_tracks_info(NULL, 1, &info) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 4;
	if (aclhip_sample_raw_scalar_tracks_batch(NULL, handles, times, 4, NULL, NULL, 48, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 5;
	if (aclhip_sample_raw_scalar_track_batch(NULL, handles, times, NULL, 4, NULL, rows, 48, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT
		|| aclhip_sample_raw_scalar_track_batch(NULL, handles, times, tracks, 4, NULL, rows, 48, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 6;
	desc.num_tracks = 3;
	desc.num_components = 4;
	desc.worst = &worst;
	if (aclhip_measure_scalar_error_batch(NULL, rows, 48, rows, 48, 1, &desc, records, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 7;
	return 0;
}
