/* aclhip_transform_compress_desc from a C99 translation unit: prints the struct's size and offsets and the new constants for
 * tests/test_transform_compress_arguments.py, and makes calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

int main(void)
{
	aclhip_transform_compress_desc desc;
	uint32_t handles[4] = { 1, 1, 1, 1 };
	memset(&desc, 0, sizeof(desc));
	printf("%u %u\n", (unsigned)sizeof(aclhip_transform_compress_desc), (unsigned)sizeof(aclhip_compress_result));
	printf("%u %u %u %u %u %u %u %u %u %u %u\n", (unsigned)offsetof(aclhip_transform_compress_desc, flags), (unsigned)offsetof(aclhip_transform_compress_desc, max_tracks),
		(unsigned)offsetof(aclhip_transform_compress_desc, default_pose), (unsigned)offsetof(aclhip_transform_compress_desc, parent_indices),
		(unsigned)offsetof(aclhip_transform_compress_desc, track_precisions), (unsigned)offsetof(aclhip_transform_compress_desc, track_shell_distances),
		(unsigned)offsetof(aclhip_transform_compress_desc, num_table_tracks), (unsigned)offsetof(aclhip_transform_compress_desc, precision),
		(unsigned)offsetof(aclhip_transform_compress_desc, shell_distance), (unsigned)offsetof(aclhip_transform_compress_desc, workspace),
		(unsigned)offsetof(aclhip_transform_compress_desc, reserved));
	printf("%u %u %u %u\n", (unsigned)ACLHIP_COMPRESS_OPTIMIZE_LOOPS, (unsigned)ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES,
		(unsigned)ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS, (unsigned)ACLHIP_COMPRESS_NOT_NORMALIZED);

	if (aclhip_transform_compress_bound(5, 7, 0) != 1536 || aclhip_transform_compress_workspace_bytes(0, 100) != 0)
		return 1;
	if (aclhip_compress_raw_tracks_batch(NULL, handles, 4, NULL, handles, 16, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	if (aclhip_compress_raw_tracks_batch(NULL, handles, 4, &desc, NULL, 16, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 3;
	return 0;
}
