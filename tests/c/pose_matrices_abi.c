/* aclhip_pose_matrices_desc and the two enums of the matrix object space from a C99 translation unit: prints the struct's size and
 * offsets for tests/test_pose_matrices_arguments.py, and makes calls that return before any device call. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "aclhip.h"

int main(void)
{
	aclhip_pose_matrices_desc desc;
	aclhip_pose_error_desc error_desc;
	aclhip_pose_error record;
	float row[16] = { 0.0f };
	float matrices[16] = { 0.0f };
	memset(&desc, 0, sizeof(desc));
	memset(&error_desc, 0, sizeof(error_desc));
	printf("%u %u %u %u %u %u\n", (unsigned)sizeof(desc), (unsigned)offsetof(aclhip_pose_matrices_desc, skeleton),
		(unsigned)offsetof(aclhip_pose_matrices_desc, instance_skeletons), (unsigned)offsetof(aclhip_pose_matrices_desc, object_space),
		(unsigned)offsetof(aclhip_pose_matrices_desc, layout), (unsigned)offsetof(aclhip_pose_matrices_desc, reserved));
	printf("%u %u %u\n", (unsigned)ACLHIP_MATRIX_3X4F_64, (unsigned)ACLHIP_METRIC_QVVF, (unsigned)ACLHIP_METRIC_QVVF_MATRIX3X4F);
	if (aclhip_pose_matrices_batch(NULL, row, 48, 1, NULL, matrices, 64, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 1;
	desc.skeleton = 1;
	desc.object_space = 1;
	desc.layout = ACLHIP_MATRIX_3X4F_64;
	if (aclhip_pose_matrices_batch(NULL, row, 48, 1, &desc, NULL, 64, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 2;
	error_desc.skeleton = 1;
	error_desc.object_space = 1;
	if (aclhip_measure_pose_error_metric_batch(NULL, row, 48, row, 48, 1, &error_desc, ACLHIP_METRIC_QVVF_MATRIX3X4F, NULL, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 3;
	if (aclhip_measure_pose_error_metric_batch(NULL, row, 48, row, 48, 1, &error_desc, 2u, &record, NULL) != ACLHIP_ERROR_INVALID_ARGUMENT)
		return 4;
	return 0;
}
