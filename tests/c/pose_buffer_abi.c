/* aclhip_pose_buffer_consumers from a C99 translation unit: prints its size and offsets for tests/test_pose_buffer_arguments.py, and
 * makes two calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

int main(void)
{
	aclhip_pose_buffer_consumers consumers;
	float row[12] = { 0.0f };
	memset(&consumers, 0, sizeof(consumers));
	printf("%u %u %u %u %u %u %u %u %u\n", (unsigned)sizeof(consumers), (unsigned)offsetof(aclhip_pose_buffer_consumers, skeleton),
		(unsigned)offsetof(aclhip_pose_buffer_consumers, instance_skeletons), (unsigned)offsetof(aclhip_pose_buffer_consumers, object_space),
		(unsigned)offsetof(aclhip_pose_buffer_consumers, additive_format), (unsigned)offsetof(aclhip_pose_buffer_consumers, additive_poses),
		(unsigned)offsetof(aclhip_pose_buffer_consumers, additive_pose_stride_bytes), (unsigned)offsetof(aclhip_pose_buffer_consumers, bounds),
		(unsigned)offsetof(aclhip_pose_buffer_consumers, reserved));
	if (aclhip_transform_poses_batch(NULL, row, 48, 1, NULL, row, 48, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 1;
	consumers.skeleton = 1;
	consumers.object_space = 1;
	if (aclhip_transform_poses_batch(NULL, NULL, 48, 1, &consumers, row, 48, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	return 0;
}
