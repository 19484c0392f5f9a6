/* aclhip_pose_bounds from a C99 translation unit: sizes and offsets for tests/test_pose_bounds_abi.py, and the argument checks of
 * aclhip_decompress_poses_batch_bounds that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

int main(void)
{
	aclhip_decompress_params params;
	aclhip_pose_consumers consumers;
	aclhip_pose_bounds bounds;
	aclhip_default_params(&params);
	memset(&consumers, 0, sizeof(consumers));
	memset(&bounds, 0, sizeof(bounds));
	consumers.object_space = 1;
	if (aclhip_decompress_poses_batch_bounds(NULL, NULL, NULL, 4, &params, &consumers, NULL, NULL, NULL, NULL, 192, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 1;
	if (aclhip_decompress_poses_batch_bounds(NULL, NULL, NULL, 4, &params, &consumers, NULL, NULL, &bounds, NULL, 192, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	if (strstr(aclhip_last_error_message(NULL), "bounds buffer") == NULL)
		return 3;
	printf("%u %u %u %u %u\n", (unsigned)sizeof(aclhip_pose_bounds), (unsigned)offsetof(aclhip_pose_bounds, bounds), (unsigned)offsetof(aclhip_pose_bounds, bone_flags),
		(unsigned)offsetof(aclhip_pose_bounds, reserved), (unsigned)ACLHIP_ABI_VERSION);
	return 0;
}
