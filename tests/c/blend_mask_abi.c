/* The blend mask declarations of include/aclhip.h from a C99 translation unit: prints sizeof(aclhip_blend_masking) and
 * sizeof(aclhip_blend_mask_info) and the offsets the binding mirrors, and makes the argument checks that need no device.
 * Exit code 0 = every check held. (tests/test_blend_mask_abi.py) */
#include <aclhip.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

int main(void)
{
	aclhip_blend_mask mask = 7;
	aclhip_blend_mask_info info;
	aclhip_blend_masking masking;
	aclhip_pose_mapping mapping;
	aclhip_pose_consumers consumers;
	aclhip_decompress_params params;
	char message[128];
	float weights[6] = { 0.0f, 1.0f, 0.5f, 1.0f, 0.25f, 0.0f };

	printf("%u %u %u %u %u %u %u %u %u %u %u %u %u\n", (unsigned)sizeof(aclhip_blend_masking), (unsigned)sizeof(aclhip_blend_mask_info),
		(unsigned)offsetof(aclhip_blend_masking, mode), (unsigned)offsetof(aclhip_blend_masking, reserved0),
		(unsigned)offsetof(aclhip_blend_masking, instance_masks), (unsigned)offsetof(aclhip_blend_masking, reserved),
		(unsigned)offsetof(aclhip_blend_mask_info, num_slots), (unsigned)offsetof(aclhip_blend_mask_info, num_zero),
		(unsigned)offsetof(aclhip_blend_mask_info, num_one), (unsigned)ACLHIP_MAX_BLEND_MASKS, (unsigned)ACLHIP_BLEND_WEIGHTED,
		(unsigned)ACLHIP_BLEND_LAYERED, (unsigned)sizeof(aclhip_blend_mask));

	memset(&masking, 0, sizeof(masking));
	memset(&mapping, 0, sizeof(mapping));
	memset(&consumers, 0, sizeof(consumers));
	aclhip_default_params(&params);
	if (aclhip_register_blend_mask(NULL, weights, 6, &mask) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 1;
	if (aclhip_unregister_blend_mask(NULL, 1) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	if (aclhip_get_blend_mask_info(NULL, 1, &info) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 3;
	if (aclhip_decompress_poses_batch_masked(NULL, NULL, NULL, 4, &params, &consumers, &mapping, &masking, NULL, 192, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 4;
	if (aclhip_check_blend_mask(weights, 6, &info, message, sizeof(message)) != ACLHIP_OK || info.num_slots != 6 || info.num_zero != 2 || info.num_one != 2)
		return 5;
	weights[4] = -0.25f;
	if (aclhip_check_blend_mask(weights, 6, &info, message, sizeof(message)) != ACLHIP_ERROR_INVALID_ARGUMENT || strstr(message, "slot 4") == NULL)
		return 6;
	if (aclhip_check_blend_mask(weights, 4, NULL, NULL, 0) != ACLHIP_OK)
		return 7;
	if (aclhip_check_blend_mask(weights, 0, NULL, NULL, 0) != ACLHIP_ERROR_INVALID_ARGUMENT || aclhip_check_blend_mask(NULL, 6, NULL, NULL, 0) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 8;
	return 0;
}
