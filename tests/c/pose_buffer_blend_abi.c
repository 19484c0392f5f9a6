/* aclhip_pose_buffer_blend from a C99 translation unit: prints its size and offsets for tests/test_pose_buffer_blend_arguments.py, and
 * makes two calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

int main(void)
{
	aclhip_pose_buffer_blend blend;
	float row[12] = { 0.0f };
	memset(&blend, 0, sizeof(blend));
	printf("%u %u %u %u %u %u %u %u %u %u %u %u %u\n", (unsigned)sizeof(blend), (unsigned)offsetof(aclhip_pose_buffer_blend, skeleton),
		(unsigned)offsetof(aclhip_pose_buffer_blend, instance_skeletons), (unsigned)offsetof(aclhip_pose_buffer_blend, num_buffers),
		(unsigned)offsetof(aclhip_pose_buffer_blend, mode), (unsigned)offsetof(aclhip_pose_buffer_blend, buffers),
		(unsigned)offsetof(aclhip_pose_buffer_blend, buffer_stride_bytes), (unsigned)offsetof(aclhip_pose_buffer_blend, weights),
		(unsigned)offsetof(aclhip_pose_buffer_blend, instance_masks), (unsigned)offsetof(aclhip_pose_buffer_blend, object_space),
		(unsigned)offsetof(aclhip_pose_buffer_blend, reserved0), (unsigned)offsetof(aclhip_pose_buffer_blend, bounds),
		(unsigned)offsetof(aclhip_pose_buffer_blend, reserved));
	if (aclhip_blend_poses_batch(NULL, NULL, 1, row, 48, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 1;
	blend.skeleton = 1;
	blend.num_buffers = 5;
	if (aclhip_blend_poses_batch(NULL, &blend, 1, row, 48, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	return 0;
}
