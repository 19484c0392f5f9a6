/* aclhip_additive_layering from a C99 translation unit: sizes and offsets for tests/test_additive_strength_abi.py, and the argument
 * checks of aclhip_decompress_poses_batch_additive_weighted that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

int main(void)
{
	aclhip_decompress_params params;
	aclhip_pose_consumers consumers;
	aclhip_pose_mapping mapping;
	aclhip_additive_layering layering;
	aclhip_default_params(&params);
	memset(&consumers, 0, sizeof(consumers));
	memset(&mapping, 0, sizeof(mapping));
	memset(&layering, 0, sizeof(layering));
	consumers.additive_format = ACLHIP_ADDITIVE_ADDITIVE1;
	if (aclhip_decompress_poses_batch_additive_weighted(NULL, NULL, NULL, 4, &params, &consumers, &mapping, NULL, NULL, 192, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 1;
	if (strstr(aclhip_last_error_message(NULL), "null additive layering") == NULL)
		return 2;
	if (aclhip_decompress_poses_batch_additive_weighted(NULL, NULL, NULL, 4, &params, &consumers, &mapping, &layering, NULL, 192, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 3;
	if (strstr(aclhip_last_error_message(NULL), "instance_weights or instance_masks") == NULL)
		return 4;
	printf("%u %u %u %u %u\n", (unsigned)sizeof(aclhip_additive_layering), (unsigned)offsetof(aclhip_additive_layering, instance_weights),
		(unsigned)offsetof(aclhip_additive_layering, instance_masks), (unsigned)offsetof(aclhip_additive_layering, reserved), (unsigned)ACLHIP_ABI_VERSION);
	return 0;
}
