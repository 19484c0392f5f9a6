/* aclhip_pose_buffer_inverse from a C99 translation unit: prints its size and offsets for tests/test_pose_buffer_inverse_arguments.py, and
 * makes two calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

int main(void)
{
	aclhip_pose_buffer_inverse inverse;
	float row[12] = { 0.0f };
	memset(&inverse, 0, sizeof(inverse));
	printf("%u %u %u %u %u %u %u %u\n", (unsigned)sizeof(inverse), (unsigned)offsetof(aclhip_pose_buffer_inverse, skeleton),
		(unsigned)offsetof(aclhip_pose_buffer_inverse, instance_skeletons), (unsigned)offsetof(aclhip_pose_buffer_inverse, local_space),
		(unsigned)offsetof(aclhip_pose_buffer_inverse, additive_format), (unsigned)offsetof(aclhip_pose_buffer_inverse, base_poses),
		(unsigned)offsetof(aclhip_pose_buffer_inverse, base_pose_stride_bytes), (unsigned)offsetof(aclhip_pose_buffer_inverse, reserved));
	if (aclhip_inverse_transform_poses_batch(NULL, row, 48, 1, NULL, row, 48, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 1;
	inverse.skeleton = 1;
	inverse.local_space = 1;
	if (aclhip_inverse_transform_poses_batch(NULL, NULL, 48, 1, &inverse, row, 48, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	return 0;
}
