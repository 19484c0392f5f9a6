/* aclhip_pose_error_desc and its records from a C99 translation unit: prints their sizes and offsets for
 * tests/test_pose_error_arguments.py, and makes two calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

int main(void)
{
	aclhip_pose_error_desc desc;
	aclhip_pose_error record;
	float row[12] = { 0.0f };
	memset(&desc, 0, sizeof(desc));
	printf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u\n", (unsigned)sizeof(desc), (unsigned)offsetof(aclhip_pose_error_desc, skeleton),
		(unsigned)offsetof(aclhip_pose_error_desc, instance_skeletons), (unsigned)offsetof(aclhip_pose_error_desc, object_space),
		(unsigned)offsetof(aclhip_pose_error_desc, additive_format), (unsigned)offsetof(aclhip_pose_error_desc, base_poses),
		(unsigned)offsetof(aclhip_pose_error_desc, base_pose_stride_bytes), (unsigned)offsetof(aclhip_pose_error_desc, shell_distances),
		(unsigned)offsetof(aclhip_pose_error_desc, num_shell_distances), (unsigned)offsetof(aclhip_pose_error_desc, shell_distance),
		(unsigned)offsetof(aclhip_pose_error_desc, bone_errors), (unsigned)offsetof(aclhip_pose_error_desc, bone_error_stride_bytes),
		(unsigned)offsetof(aclhip_pose_error_desc, worst), (unsigned)offsetof(aclhip_pose_error_desc, reserved));
	printf("%u %u %u %u %u %u %u %u\n", (unsigned)sizeof(aclhip_pose_error), (unsigned)offsetof(aclhip_pose_error, error), (unsigned)offsetof(aclhip_pose_error, bone),
		(unsigned)sizeof(aclhip_pose_error_worst), (unsigned)offsetof(aclhip_pose_error_worst, error), (unsigned)offsetof(aclhip_pose_error_worst, bone),
		(unsigned)offsetof(aclhip_pose_error_worst, instance), (unsigned)offsetof(aclhip_pose_error_worst, reserved));
	if (ACLHIP_NO_BONE != 0xFFFFFFFFu)
		return 3;
	if (aclhip_measure_pose_error_batch(NULL, row, 48, row, 48, 1, NULL, &record, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 1;
	desc.skeleton = 1;
	desc.object_space = 1;
	if (aclhip_measure_pose_error_batch(NULL, row, 48, row, 48, 1, &desc, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	return 0;
}
