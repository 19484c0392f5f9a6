/* aclhip_raw_tracks_info and aclhip_raw_sample_desc from a C99 translation unit: prints the structs' sizes and offsets for
 * tests/test_raw_tracks_abi.py, and makes calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

int main(void)
{
	aclhip_raw_sample_desc desc;
	aclhip_raw_tracks_info info;
	aclhip_raw_tracks raw = 99;
	char message[128];
	float samples[24] = { 0.0f };
	uint32_t handles[4] = { 1, 1, 1, 1 };
	float times[4] = { 0.0f };
	float rows[48] = { 0.0f };
	memset(&desc, 0, sizeof(desc));
	printf("%u %u\n", (unsigned)sizeof(aclhip_raw_sample_desc), (unsigned)sizeof(aclhip_raw_tracks_info));
	printf("%u %u %u %u %u %u %u %u\n", (unsigned)offsetof(aclhip_raw_sample_desc, rounding_policy), (unsigned)offsetof(aclhip_raw_sample_desc, reserved0),
		(unsigned)offsetof(aclhip_raw_sample_desc, instance_rounding_policies), (unsigned)offsetof(aclhip_raw_sample_desc, track_rounding_policies),
		(unsigned)offsetof(aclhip_raw_sample_desc, num_track_rounding_policies), (unsigned)offsetof(aclhip_raw_sample_desc, reserved1),
		(unsigned)offsetof(aclhip_raw_sample_desc, rows), (unsigned)offsetof(aclhip_raw_sample_desc, reserved));
	printf("%u %u %u %u %u %u\n", (unsigned)offsetof(aclhip_raw_tracks_info, num_tracks), (unsigned)offsetof(aclhip_raw_tracks_info, num_samples),
		(unsigned)offsetof(aclhip_raw_tracks_info, sample_rate), (unsigned)offsetof(aclhip_raw_tracks_info, duration),
		(unsigned)offsetof(aclhip_raw_tracks_info, looping_policy), (unsigned)offsetof(aclhip_raw_tracks_info, reserved));
	printf("%u %u\n", (unsigned)ACLHIP_MAX_RAW_TRACKS, (unsigned)sizeof(aclhip_raw_tracks));

	if (aclhip_check_raw_tracks(samples, 1, 2, 30.0f, ACLHIP_LOOP_WRAP, &info, message, sizeof(message)) != ACLHIP_OK || info.num_samples != 2 || info.looping_policy != ACLHIP_LOOP_WRAP)
		return 1;
	if (aclhip_check_raw_tracks(samples, 1, 2, 0.0f, ACLHIP_LOOP_CLAMP, &info, message, sizeof(message)) != ACLHIP_ERROR_INVALID_ARGUMENT || strstr(message, "sample rate") == NULL)
		return 2;
	if (aclhip_register_raw_tracks(NULL, samples, 1, 2, 30.0f, ACLHIP_LOOP_CLAMP, &raw) != ACLHIP_ERROR_INVALID_ARGUMENT || raw != 0)
		return 3;
	if (aclhip_unregister_raw_tracks(NULL, 1) != ACLHIP_ERROR_INVALID_ARGUMENT || aclhip_get_raw_tracks_info(NULL, 1, &info) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 4;
	if (aclhip_sample_raw_tracks_batch(NULL, handles, times, 4, NULL, NULL, 48, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 5;
	desc.rounding_policy = ACLHIP_ROUND_PER_TRACK;
	if (aclhip_sample_raw_tracks_batch(NULL, handles, times, 4, &desc, rows, 48, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 6;
	return 0;
}
