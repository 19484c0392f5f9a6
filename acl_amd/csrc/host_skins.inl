// host_skins.inl -- part of aclhip.hip (one translation unit; included there behind host_pose_buffers.inl, not compiled on its own).
// Host side: skins (a mesh's joint list and inverse bind matrices) -- what registration checks, the record and its image; the handles are
// a handle_table's (host_context.inl) -- and aclhip_skinning_matrices_batch (skinning_matrices_kernel, kernels_pose_buffers.inl): its
// own argument check and kernel argument behind what host_pose_buffers.inl states for every launch over a caller's pose rows.

namespace
{
	// What registration checks; the message names the first offending joint
	bool check_skin(const uint32_t* joint_bones, const float* inverse_bind, uint32_t num_joints, uint32_t num_bones, aclhip_skin_info& info, char* message, size_t capacity)
	{
		const auto say = [&](const char* format, uint32_t a, uint32_t b, uint32_t c)
		{
			if (message != nullptr && capacity != 0)
				std::snprintf(message, capacity, format, a, b, c);
			return false;
		};
		if (message != nullptr && capacity != 0)
			message[0] = '\0';
		std::memset(&info, 0, sizeof(info));
		if (num_joints == 0)
			return say("a skin of %u joints", num_joints, 0, 0);
		if (num_joints > 0xFFFFu)
			return say("%u joints: a skin holds at most 65535", num_joints, 0, 0);
		if (num_bones == 0)
			return say("a skin for a skeleton of %u bones", num_bones, 0, 0);
		if (num_bones > 0xFFFFu)
			return say("%u bones: a skeleton holds at most 65535", num_bones, 0, 0);
		if (joint_bones == nullptr && num_joints != num_bones)
			return say("null joint bones (the identity list) with %u joints for %u bones", num_joints, num_bones, 0);

		bool is_identity = num_joints == num_bones;
		for (uint32_t joint = 0; joint < num_joints; ++joint)
		{
			const uint32_t bone = joint_bones != nullptr ? joint_bones[joint] : joint;
			if (bone >= num_bones)
				return say("joint %u: bone %u is outside the skeleton's %u bones", joint, bone, num_bones);
			is_identity = is_identity && bone == joint;
			if (inverse_bind != nullptr)
			{
				for (uint32_t axis = 0; axis < 4; ++axis)
					for (uint32_t lane = 0; lane < 3; ++lane)
						if (!std::isfinite(inverse_bind[size_t(joint) * 16 + axis * 4 + lane]))
							return say("joint %u: lane %u of axis %u of its inverse bind matrix is not finite", joint, lane, axis);
			}
		}
		info.num_joints = num_joints;
		info.num_bones = num_bones;
		info.is_identity_joint_list = is_identity ? 1u : 0u;
		info.has_inverse_bind = inverse_bind != nullptr ? 1u : 0u;
		return true;
	}
}

extern "C" aclhip_status aclhip_check_skin(const uint32_t* joint_bones, const float* inverse_bind, uint32_t num_joints, uint32_t num_bones, aclhip_skin_info* out_info,
	char* message, uint32_t message_capacity)
{
	return guarded(static_cast<aclhip_context*>(nullptr), [&]() -> aclhip_status
	{
		aclhip_skin_info info;
		const bool valid = check_skin(joint_bones, inverse_bind, num_joints, num_bones, info, message, message_capacity);
		if (valid && out_info != nullptr)
			*out_info = info;
		return valid ? ACLHIP_OK : ACLHIP_ERROR_INVALID_ARGUMENT;
	});
}

extern "C" aclhip_status aclhip_register_skin(aclhip_context* context, const uint32_t* joint_bones, const float* inverse_bind, uint32_t num_joints, uint32_t num_bones,
	aclhip_skin* out_skin)
{
	if (context == nullptr || out_skin == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	*out_skin = 0;
	return guarded(context, [&]() -> aclhip_status
	{
		// (everything that needs no device first: a refused skin makes no HIP call)
		aclhip_skin_info info;
		char message[256];
		if (!check_skin(joint_bones, inverse_bind, num_joints, num_bones, info, message, sizeof(message)))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s", message);

		// the device image: the matrices, twelve floats per joint in the three quads load_matrix reads, and the joint list behind them
		const size_t matrix_bytes = size_t(num_joints) * 48, image_bytes = matrix_bytes + size_t(num_joints) * sizeof(uint32_t);
		std::vector<uint32_t> image(image_bytes / sizeof(uint32_t));
		float* matrices = reinterpret_cast<float*>(image.data());
		for (uint32_t joint = 0; joint < num_joints; ++joint)
		{
			for (uint32_t axis = 0; axis < 4; ++axis)
				for (uint32_t lane = 0; lane < 3; ++lane)
					matrices[size_t(joint) * 12 + axis * 3 + lane] = inverse_bind != nullptr ? inverse_bind[size_t(joint) * 16 + axis * 4 + lane] : (axis == lane ? 1.0f : 0.0f);
			image[size_t(num_joints) * 12 + joint] = joint_bones != nullptr ? joint_bones[joint] : joint;
		}

		std::lock_guard<std::shared_mutex> lock(context->mutex);
		device_guard guard(context->device);
		collect_retired(context, false);

		uint32_t slot;
		if (const aclhip_status status = take_handle(context, context->skins, slot); status != ACLHIP_OK)
			return status;

		// (a piece of a clip slab, uploaded on the context's copy stream: no allocation call and no copy that would stall the device)
		uint8_t* d_image = allocate_clip_memory(context, image_bytes);
		if (d_image == nullptr)
		{
			context->skins.give_back(slot);
			return fail(context, ACLHIP_ERROR_OUT_OF_MEMORY, "allocating %zu bytes for the skin failed", image_bytes);
		}
		device_skin record;
		std::memset(&record, 0, sizeof(record));
		record.inverse_bind = reinterpret_cast<const f32x4*>(d_image);
		record.joint_bones = reinterpret_cast<const uint32_t*>(d_image + matrix_bytes);
		record.num_joints = num_joints;
		record.num_bones = num_bones;
		record.flags = (info.is_identity_joint_list != 0 ? k_skin_identity_joint_list : 0u) | (info.has_inverse_bind != 0 ? k_skin_has_inverse_bind : 0u);
		size_t staging_used = 0;
		// the image first, the record that publishes it behind it
		if (!stage_upload(context, d_image, image.data(), image_bytes, staging_used)
			|| !publish_handle(context, context->skins, slot, record, staging_used, info, d_image))
		{
			free_clip_memory(context, d_image);
			context->skins.give_back(slot);
			return fail(context, ACLHIP_ERROR_DEVICE, "uploading the skin failed");
		}
		*out_skin = slot;
		return ACLHIP_OK;
	});
}

extern "C" aclhip_status aclhip_unregister_skin(aclhip_context* context, aclhip_skin skin)
{
	if (context == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return unregister_handle(context, context->skins, skin);
}

extern "C" aclhip_status aclhip_get_skin_info(const aclhip_context* context, aclhip_skin skin, aclhip_skin_info* out_info)
{
	if (context == nullptr || out_info == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return get_handle_info(context, context->skins, skin, out_info);
}

namespace
{
	// ---- skinning matrix palettes of a pose buffer (aclhip_skinning_matrices_batch; skinning_matrices_kernel) ------------------------------

	// What aclhip_skinning_matrices_batch checks of its arguments before any device call; every refusal leaves a message, with or without a
	// context. The rows that shape the launch: the pose row alone -- an image holds pose_stride_bytes / 48 transforms (a palette row has as
	// many records as the skin has joints, which says nothing about the image).
	aclhip_status check_skinning_matrices(aclhip_context* context, const void* poses, uint64_t pose_stride_bytes, uint32_t num_instances, const aclhip_skinning_desc* desc,
		const void* palettes, uint64_t palette_stride_bytes, pose_rows& out_rows)
	{
		if (desc == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null skinning desc");
		if (poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose buffer");
		if (palettes == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null palette buffer");
		if (const aclhip_status status = check_names_skeleton(context, "a skinning desc names", desc->skeleton, desc->instance_skeletons); status != ACLHIP_OK)
			return status;
		if (desc->skin == 0 && desc->instance_skins == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a skinning desc names a skin or a list of skins");
		if (desc->layout != ACLHIP_PALETTE_3X4F_64 && desc->layout != ACLHIP_PALETTE_3X4F_TRANSPOSED_48)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown palette layout %u", desc->layout);
		if (const aclhip_status status = check_rows_aligned(context, { { "pose", poses, pose_stride_bytes }, { "palette", palettes, palette_stride_bytes } }); status != ACLHIP_OK)
			return status;
		if (desc->reserved[0] != 0 || desc->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a skinning desc are 0");
		out_rows = { pose_stride_bytes / 48, false, "too large for the skinning matrices" };
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_rows_launch_shape_of(context, out_rows, false, 0, shape); shape_status != ACLHIP_OK)
			return shape_status;
		// records differ from transforms in size and in number: there is no in place form, and no other overlap either (the lists are only read as well)
		if (pose_ranges_overlap(palettes, palette_stride_bytes, poses, pose_stride_bytes, num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the palette rows overlap the pose rows: there is no in place form");
		if (desc->instance_skeletons != nullptr && pose_ranges_overlap(palettes, palette_stride_bytes, desc->instance_skeletons, sizeof(aclhip_skeleton), num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the palette rows overlap the skeleton list");
		if (desc->instance_skins != nullptr && pose_ranges_overlap(palettes, palette_stride_bytes, desc->instance_skins, sizeof(aclhip_skin), num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the palette rows overlap the skin list");
		return ACLHIP_OK;
	}
}

// include/aclhip.h states the definition. The argument checks need no device, come first and leave a message, with or without a context.
// The front is launch_pose_rows (host_pose_buffers.inl), which asks for the skin table as well.
extern "C" aclhip_status aclhip_skinning_matrices_batch(aclhip_context* context, const void* poses, uint64_t pose_stride_bytes, uint32_t num_instances,
	const aclhip_skinning_desc* desc, void* palettes, uint64_t palette_stride_bytes, void* stream_handle)
{
	pose_rows rows;
	const aclhip_status status = check_skinning_matrices(context, poses, pose_stride_bytes, num_instances, desc, palettes, palette_stride_bytes, rows);
	if (status != ACLHIP_OK)
		return status;
	const bool object_space = desc->object_space != 0;
	return launch_pose_rows(context, num_instances, stream_handle, rows, object_space, true, false, [&](hipStream_t stream, const consumer_launch_shape& shape, uint32_t num_blocks) -> aclhip_status
	{
		skinning_matrices_launch launch = {};
		launch.head = pose_rows_head_of(context, desc->skeleton, desc->instance_skeletons);
		launch.shape = pose_rows_shape_of(context, num_instances, shape);
		launch.skins = context->skins.d_records;
		launch.num_skins = ACLHIP_MAX_SKINS;
		launch.skin = desc->skin;
		launch.instance_skins = desc->instance_skins;
		launch.poses = static_cast<const uint8_t*>(poses);
		launch.pose_stride_bytes = pose_stride_bytes;
		launch.palettes = static_cast<uint8_t*>(palettes);
		launch.palette_stride_bytes = palette_stride_bytes;

		const bool transposed = desc->layout == ACLHIP_PALETTE_3X4F_TRANSPOSED_48;
		const auto kernel = object_space
			? (transposed ? skinning_matrices_kernel<true, k_palette_3x4f_transposed_48> : skinning_matrices_kernel<true, k_palette_3x4f_64>)
			: (transposed ? skinning_matrices_kernel<false, k_palette_3x4f_transposed_48> : skinning_matrices_kernel<false, k_palette_3x4f_64>);
		return launch_consumer_kernel(context, kernel, shape, num_blocks, 1, stream, launch);
	});
}
