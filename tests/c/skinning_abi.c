/* aclhip_skin_info, aclhip_skinning_desc and aclhip_palette_layout from a C99 translation unit: prints the structs' sizes and offsets for
 * tests/test_skin_abi.py, and makes calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

int main(void)
{
	aclhip_skinning_desc desc;
	aclhip_skin_info info;
	aclhip_skin skin = 99;
	char message[128];
	uint32_t joints[2] = { 1, 0 };
	float bind[32] = { 0.0f };
	float row[24] = { 0.0f };
	float palette[32] = { 0.0f };
	memset(&desc, 0, sizeof(desc));
	printf("%u %u\n", (unsigned)sizeof(aclhip_skinning_desc), (unsigned)sizeof(aclhip_skin_info));
	printf("%u %u %u %u %u %u %u\n", (unsigned)offsetof(aclhip_skinning_desc, skeleton), (unsigned)offsetof(aclhip_skinning_desc, instance_skeletons),
		(unsigned)offsetof(aclhip_skinning_desc, skin), (unsigned)offsetof(aclhip_skinning_desc, instance_skins), (unsigned)offsetof(aclhip_skinning_desc, object_space),
		(unsigned)offsetof(aclhip_skinning_desc, layout), (unsigned)offsetof(aclhip_skinning_desc, reserved));
	printf("%u %u %u %u %u\n", (unsigned)offsetof(aclhip_skin_info, num_joints), (unsigned)offsetof(aclhip_skin_info, num_bones),
		(unsigned)offsetof(aclhip_skin_info, is_identity_joint_list), (unsigned)offsetof(aclhip_skin_info, has_inverse_bind), (unsigned)offsetof(aclhip_skin_info, reserved));
	printf("%u %u %u %u\n", (unsigned)ACLHIP_MAX_SKINS, (unsigned)ACLHIP_PALETTE_3X4F_64, (unsigned)ACLHIP_PALETTE_3X4F_TRANSPOSED_48, (unsigned)sizeof(aclhip_skin));

	if (aclhip_check_skin(joints, bind, 2, 2, &info, message, sizeof(message)) != ACLHIP_OK || info.num_joints != 2 || info.is_identity_joint_list != 0)
		return 1;
	joints[1] = 2;
	if (aclhip_check_skin(joints, bind, 2, 2, &info, message, sizeof(message)) != ACLHIP_ERROR_INVALID_ARGUMENT || strstr(message, "joint 1") == NULL)
		return 2;
	if (aclhip_register_skin(NULL, NULL, NULL, 2, 2, &skin) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 3;
	if (aclhip_unregister_skin(NULL, 1) != ACLHIP_ERROR_INVALID_ARGUMENT || aclhip_get_skin_info(NULL, 1, &info) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 4;
	if (aclhip_skinning_matrices_batch(NULL, row, 96, 1, NULL, palette, 128, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 5;
	desc.skeleton = 1;
	desc.skin = 1;
	desc.object_space = 1;
	desc.layout = ACLHIP_PALETTE_3X4F_TRANSPOSED_48;
	if (aclhip_skinning_matrices_batch(NULL, row, 96, 1, &desc, NULL, 96, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 6;
	return 0;
}
