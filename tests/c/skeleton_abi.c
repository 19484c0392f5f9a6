/* The skeleton declarations of include/aclhip.h from a C99 translation unit: prints sizeof(aclhip_pose_mapping) and
 * sizeof(aclhip_skeleton_info) and the offsets the binding mirrors, and makes the argument checks that need no device.
 * Exit code 0 = every check held. (tests/test_skeleton_abi.py) */
#include <aclhip.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

int main(void)
{
	aclhip_skeleton skeleton = 7;
	aclhip_skeleton_info info;
	aclhip_pose_mapping mapping;
	aclhip_pose_consumers consumers;
	aclhip_decompress_params params;
	char message[128];
	const uint32_t parents[4] = { ACLHIP_NO_PARENT, 0, 1, 1 };
	const uint32_t child_first[4] = { ACLHIP_NO_PARENT, 2, 0, 1 };
	float pose[4 * 12];
	int bone;

	printf("%u %u %u %u %u %u %u %u %u %u %u\n", (unsigned)sizeof(aclhip_pose_mapping), (unsigned)sizeof(aclhip_skeleton_info),
		(unsigned)offsetof(aclhip_pose_mapping, skeleton), (unsigned)offsetof(aclhip_pose_mapping, instance_skeletons),
		(unsigned)offsetof(aclhip_pose_mapping, map), (unsigned)offsetof(aclhip_pose_mapping, instance_maps),
		(unsigned)offsetof(aclhip_pose_mapping, blend_maps), (unsigned)offsetof(aclhip_pose_mapping, base_maps),
		(unsigned)offsetof(aclhip_skeleton_info, walk_steps), (unsigned)offsetof(aclhip_skeleton_info, has_negative_scale),
		(unsigned)ACLHIP_MAX_SKELETONS);

	memset(pose, 0, sizeof(pose));
	for (bone = 0; bone < 4; ++bone)
		pose[bone * 12 + 3] = pose[bone * 12 + 8] = pose[bone * 12 + 9] = pose[bone * 12 + 10] = 1.0f;
	memset(&mapping, 0, sizeof(mapping));
	memset(&consumers, 0, sizeof(consumers));
	aclhip_default_params(&params);
	if (aclhip_register_skeleton(NULL, parents, pose, 4, &skeleton) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 1;
	if (aclhip_unregister_skeleton(NULL, 1) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	if (aclhip_get_skeleton_info(NULL, 1, &info) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 3;
	if (aclhip_decompress_poses_batch_mapped(NULL, NULL, NULL, 4, &params, &consumers, &mapping, NULL, 192, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 4;
	if (aclhip_check_skeleton(parents, pose, 4, &info, message, sizeof(message)) != ACLHIP_OK || info.num_bones != 4 || info.has_hierarchy != 1
		|| info.num_roots != 1 || info.depth != 3 || info.walk_steps != 2 || info.has_negative_scale != 0)
		return 5;
	if (aclhip_check_skeleton(child_first, pose, 4, &info, message, sizeof(message)) != ACLHIP_ERROR_INVALID_ARGUMENT || strstr(message, "bone 1") == NULL)
		return 6;
	if (aclhip_check_skeleton(NULL, pose, 4, &info, NULL, 0) != ACLHIP_OK || info.has_hierarchy != 0 || info.walk_steps != 0)
		return 7;
	if (aclhip_check_skeleton(parents, pose, 0, NULL, NULL, 0) != ACLHIP_ERROR_INVALID_ARGUMENT || aclhip_check_skeleton(parents, NULL, 4, NULL, NULL, 0) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 8;
	pose[2 * 12 + 9] = -1.0f;
	if (aclhip_check_skeleton(parents, pose, 4, &info, NULL, 0) != ACLHIP_OK || info.has_negative_scale != 1)
		return 9;
	return 0;
}
