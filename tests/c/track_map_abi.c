/* The track map declarations of include/aclhip.h from a C99 translation unit: prints sizeof(aclhip_track_mapping) and
 * sizeof(aclhip_track_map_info) and the offsets the binding mirrors, and makes the argument checks that need no device.
 * Exit code 0 = every check held. (tests/test_track_map_abi.py) */
#include <aclhip.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

int main(void)
{
	aclhip_track_map map = 7;
	aclhip_track_map_info info;
	aclhip_track_mapping mapping;
	aclhip_decompress_params params;
	char message[128];
	const uint32_t identity[3] = { 0, 1, 2 };
	const uint32_t duplicate[3] = { 0, 1, 1 };
	const uint32_t with_drop[3] = { 4, ACLHIP_TRACK_DROPPED, 2 };

	printf("%u %u %u %u %u %u\n", (unsigned)sizeof(aclhip_track_mapping), (unsigned)sizeof(aclhip_track_map_info),
		(unsigned)offsetof(aclhip_track_mapping, map), (unsigned)offsetof(aclhip_track_mapping, instance_maps),
		(unsigned)offsetof(aclhip_track_mapping, fill_pose), (unsigned)offsetof(aclhip_track_mapping, fill_unmapped));

	memset(&mapping, 0, sizeof(mapping));
	aclhip_default_params(&params);
	if (aclhip_register_track_map(NULL, identity, 3, 3, &map) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 1;
	if (aclhip_unregister_track_map(NULL, 1) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	if (aclhip_get_track_map_info(NULL, 1, &info) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 3;
	if (aclhip_decompress_tracks_batch_mapped(NULL, NULL, NULL, 4, &params, NULL, &mapping, NULL, 4800, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 4;
	if (aclhip_check_track_map(identity, 3, 3, &info, message, sizeof(message)) != ACLHIP_OK || info.is_identity != 1 || info.num_unmapped_slots != 0)
		return 5;
	if (aclhip_check_track_map(duplicate, 3, 3, &info, message, sizeof(message)) != ACLHIP_ERROR_INVALID_ARGUMENT || strstr(message, "track 2") == NULL)
		return 6;
	if (aclhip_check_track_map(with_drop, 3, 5, &info, NULL, 0) != ACLHIP_OK || info.num_dropped != 1 || info.num_mapped != 2 || info.num_unmapped_slots != 3
		|| info.is_order_preserving != 0 || info.is_identity != 0)
		return 7;
	if (aclhip_check_track_map(identity, 0, 3, NULL, NULL, 0) != ACLHIP_ERROR_INVALID_ARGUMENT || aclhip_check_track_map(identity, 3, 0, NULL, NULL, 0) != ACLHIP_ERROR_INVALID_ARGUMENT
		|| aclhip_check_track_map(NULL, 3, 3, NULL, NULL, 0) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 8;
	return 0;
}
