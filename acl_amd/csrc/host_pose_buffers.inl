// host_pose_buffers.inl -- part of aclhip.hip (one translation unit; included there, in this order, not compiled on its own).
// Host side: the pose consumers over a caller's pose buffers (aclhip_transform_poses_batch, aclhip_blend_poses_batch,
// aclhip_inverse_transform_poses_batch, aclhip_measure_pose_error_batch and its _metric form, aclhip_pose_matrices_batch;
// kernels_pose_buffers.inl).

namespace
{
	// The rows alone set the shape of the launch (the output rows when there are any): an image's quads, and the words of the walk schedule on
	// top of them once the context is known (launch_pose_buffers; the argument check asks without them). Refuses rows that do not fit.
	aclhip_status pose_buffer_launch_shape_of(aclhip_context* context, const void* poses, uint64_t pose_stride_bytes, uint64_t local_pose_stride_bytes, bool object_space,
		uint32_t max_hierarchy_words, consumer_launch_shape& out_shape)
	{
		const uint64_t shape_stride_bytes = poses != nullptr ? pose_stride_bytes : local_pose_stride_bytes;
		const uint32_t row_transforms = uint32_t(std::min<uint64_t>(shape_stride_bytes / 48, 0xFFFFu));
		out_shape = consumer_launch_shape_of(row_transforms * 3u, row_transforms, false, object_space, max_hierarchy_words);
		if (!out_shape.fits)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "rows of %u transforms: too large for the pose consumers (%zu bytes of LDS per instance)", row_transforms, out_shape.lds_needed_bytes);
		return ACLHIP_OK;
	}

	// What aclhip_transform_poses_batch checks of its arguments before any device call; every refusal leaves a message, with or without a context
	aclhip_status check_pose_buffer_consumers(aclhip_context* context, const void* local_poses, uint64_t local_pose_stride_bytes, uint32_t num_instances,
		const aclhip_pose_buffer_consumers* consumers, const void* poses, uint64_t pose_stride_bytes)
	{
		if (consumers == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose buffer consumers");
		if (local_poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null local pose buffer");
		if (consumers->skeleton == 0 && consumers->instance_skeletons == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose buffer consumers name a skeleton or a list of skeletons");
		if (consumers->additive_format > ACLHIP_ADDITIVE_ADDITIVE1)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown additive format %u", consumers->additive_format);
		const bool has_additive = consumers->additive_format != ACLHIP_ADDITIVE_NONE;
		if (consumers->object_space == 0 && !has_additive)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "neither object_space nor an additive format: nothing to do");
		if (has_additive != (consumers->additive_poses != nullptr))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "an additive format and an additive pose buffer come together");
		if (consumers->bounds != nullptr && consumers->object_space == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose bounds are taken in object space: a local space translation is not a position");
		if (poses == nullptr && consumers->bounds == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null output buffer without bounds");
		if ((local_pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(local_poses) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "local pose buffer and stride must be 16 byte aligned");
		if ((pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(poses) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose buffer and stride must be 16 byte aligned");
		if (has_additive && ((consumers->additive_pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(consumers->additive_poses) & 15u) != 0))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "additive pose buffer and stride must be 16 byte aligned");
		if (consumers->reserved[0] != 0 || consumers->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of pose buffer consumers are 0");
		if (consumers->bounds != nullptr)
			if (const aclhip_status bounds_status = check_pose_bounds(context, consumers->bounds); bounds_status != ACLHIP_OK)
				return bounds_status;
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_buffer_launch_shape_of(context, poses, pose_stride_bytes, local_pose_stride_bytes, false, 0, shape); shape_status != ACLHIP_OK)
			return shape_status;
		// in place is the one overlap allowed: a wave reads its own instance's rows and has them complete in LDS before it stores
		if (poses != nullptr)
		{
			const bool in_place = poses == local_poses && pose_stride_bytes == local_pose_stride_bytes;
			if (!in_place && pose_ranges_overlap(poses, pose_stride_bytes, local_poses, local_pose_stride_bytes, num_instances))
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the output rows overlap the local pose rows: only poses == local_poses with equal strides (in place) is allowed");
			if (has_additive && pose_ranges_overlap(poses, pose_stride_bytes, consumers->additive_poses, consumers->additive_pose_stride_bytes, num_instances))
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the output rows overlap the additive pose rows");
		}
		return ACLHIP_OK;
	}

	template<bool kObjectSpace, uint32_t kBase, class... bounds_types>
	aclhip_status launch_transform_poses_kernel(aclhip_context* context, const consumer_launch_shape& shape, uint32_t num_blocks, hipStream_t stream, const pose_buffer_launch& launch, const bounds_types&... bounds)
	{
		const auto kernel = transform_poses_kernel<kObjectSpace, kBase, bounds_types...>;
		// above the default limit of dynamic LDS the kernel has to be told
		if (shape.lds_bytes > 64 * 1024 - 128)
			ACLHIP_CHECK_HIP(context, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(k_consumer_lds_bytes)));
		hipLaunchKernelGGL(kernel, dim3(num_blocks), dim3((1u << shape.log2_instances_per_block) * k_wave_size), shape.lds_bytes, stream, launch, bounds...);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
		return ACLHIP_OK;
	}

	// The launch: shaped by its rows alone, like the mapped launch (registered clips play no part); the skeleton table is filled in under
	// the registry lock, as launch_consumers does it; nothing is uploaded
	aclhip_status launch_pose_buffers(aclhip_context* context, const void* local_poses, uint64_t local_pose_stride_bytes, uint32_t num_instances,
		const aclhip_pose_buffer_consumers& consumers, void* poses, uint64_t pose_stride_bytes, hipStream_t stream)
	{
		std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
		if (context->skeletons.d_records == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no skeleton was ever registered with this context");
		const bool object_space = consumers.object_space != 0;
		const bool has_additive = consumers.additive_format != ACLHIP_ADDITIVE_NONE;
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_buffer_launch_shape_of(context, poses, pose_stride_bytes, local_pose_stride_bytes, object_space, context->max_skeleton_hierarchy_words, shape); shape_status != ACLHIP_OK)
			return shape_status;
		note_launch_stream(context, stream);

		pose_buffer_launch launch = {};
		launch.skeletons = context->skeletons.d_records;
		launch.num_skeletons = ACLHIP_MAX_SKELETONS;
		launch.skeleton = consumers.skeleton;
		launch.instance_skeletons = consumers.instance_skeletons;
		launch.local_poses = static_cast<const uint8_t*>(local_poses);
		launch.local_pose_stride_bytes = local_pose_stride_bytes;
		launch.additive_poses = has_additive ? static_cast<const uint8_t*>(consumers.additive_poses) : nullptr;
		launch.additive_pose_stride_bytes = has_additive ? consumers.additive_pose_stride_bytes : 0;
		launch.poses = static_cast<uint8_t*>(poses);
		launch.pose_stride_bytes = pose_stride_bytes;
		launch.num_instances = num_instances;
		launch.additive_format = consumers.additive_format;
		launch.lds_quads_per_image = shape.lds_quads_per_image;
		launch.lds_bytes_per_instance = uint32_t(shape.lds_bytes_per_instance);
		launch.packed_block_shape = shape.log2_instances_per_block | (shape.lds_schedule_words << 8);
		launch.rejected_count = context->d_rejected;

		const uint32_t instances_per_block = 1u << shape.log2_instances_per_block;
		const uint32_t num_blocks = (num_instances + instances_per_block - 1) / instances_per_block;
		// five instantiations: object / none, object / buffer, local / buffer, and the two object forms with bounds
		if (consumers.bounds != nullptr)
		{
			const consumer_bounds_launch bounds = { static_cast<uint8_t*>(consumers.bounds->bounds), consumers.bounds->bone_flags };
			return has_additive ? launch_transform_poses_kernel<true, k_consumer_base_buffer>(context, shape, num_blocks, stream, launch, bounds)
				: launch_transform_poses_kernel<true, k_consumer_base_none>(context, shape, num_blocks, stream, launch, bounds);
		}
		if (!object_space)
			return launch_transform_poses_kernel<false, k_consumer_base_buffer>(context, shape, num_blocks, stream, launch);
		return has_additive ? launch_transform_poses_kernel<true, k_consumer_base_buffer>(context, shape, num_blocks, stream, launch)
			: launch_transform_poses_kernel<true, k_consumer_base_none>(context, shape, num_blocks, stream, launch);
	}

	// ---- a blend of K caller pose buffers (aclhip_blend_poses_batch; blend_poses_kernel in kernels_pose_buffers.inl) ----------------------

	// What aclhip_blend_poses_batch checks of its arguments before any device call; every refusal leaves a message, with or without a context
	aclhip_status check_pose_buffer_blend(aclhip_context* context, const aclhip_pose_buffer_blend* blend, uint32_t num_instances, const void* poses, uint64_t pose_stride_bytes)
	{
		if (blend == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose buffer blend");
		const uint32_t num_buffers = blend->num_buffers;
		if (num_buffers < 2 || num_buffers > ACLHIP_MAX_BLEND_CLIPS)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a blend of %u pose buffers: 2 to %u", num_buffers, ACLHIP_MAX_BLEND_CLIPS);
		if (blend->mode > ACLHIP_BLEND_LAYERED)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown blend mode %u", blend->mode);
		for (uint32_t k = 0; k < ACLHIP_MAX_BLEND_CLIPS; ++k)
		{
			if (k < num_buffers && blend->buffers[k] == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose buffer %u of the blend's %u is null", k, num_buffers);
			if (k >= num_buffers && blend->buffers[k] != nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose buffer %u is set in a blend of %u: entries behind the blend are null", k, num_buffers);
		}
		if (blend->weights == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a pose buffer blend needs weights");
		if (blend->skeleton == 0 && blend->instance_skeletons == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a pose buffer blend names a skeleton or a list of skeletons");
		if (blend->bounds != nullptr && blend->object_space == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose bounds are taken in object space: a local space translation is not a position");
		if (poses == nullptr && blend->bounds == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null output buffer without bounds");
		for (uint32_t k = 0; k < num_buffers; ++k)
			if ((blend->buffer_stride_bytes[k] & 15u) != 0 || (reinterpret_cast<uintptr_t>(blend->buffers[k]) & 15u) != 0)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose buffer %u and its stride must be 16 byte aligned", k);
		if ((pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(poses) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose buffer and stride must be 16 byte aligned");
		if (blend->reserved0 != 0 || blend->reserved[0] != 0 || blend->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a pose buffer blend are 0");
		if (blend->bounds != nullptr)
			if (const aclhip_status bounds_status = check_pose_bounds(context, blend->bounds); bounds_status != ACLHIP_OK)
				return bounds_status;
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_buffer_launch_shape_of(context, poses, pose_stride_bytes, blend->buffer_stride_bytes[0], false, 0, shape); shape_status != ACLHIP_OK)
			return shape_status;
		// in place on ONE input is the one overlap allowed: a wave reads its own instance's rows and has the blend complete in LDS before it
		// stores. The inputs are only read: they may overlap each other.
		for (uint32_t k = 0; k < num_buffers && poses != nullptr; ++k)
		{
			const bool in_place = poses == blend->buffers[k] && pose_stride_bytes == blend->buffer_stride_bytes[k];
			if (!in_place && pose_ranges_overlap(poses, pose_stride_bytes, blend->buffers[k], blend->buffer_stride_bytes[k], num_instances))
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the output rows overlap the rows of pose buffer %u: only poses == buffers[k] with equal strides (in place) is allowed", k);
		}
		if (blend->bounds != nullptr)
		{
			const void* boxes = blend->bounds->bounds;
			if (poses != nullptr && pose_ranges_overlap(boxes, 32, poses, pose_stride_bytes, num_instances))
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the bounds overlap the output rows");
			for (uint32_t k = 0; k < num_buffers; ++k)
				if (pose_ranges_overlap(boxes, 32, blend->buffers[k], blend->buffer_stride_bytes[k], num_instances))
					return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the bounds overlap the rows of pose buffer %u", k);
		}
		return ACLHIP_OK;
	}

	template<uint32_t kNumBuffers, bool kObjectSpace, class... bounds_types>
	aclhip_status launch_blend_poses_kernel(aclhip_context* context, const consumer_launch_shape& shape, uint32_t num_blocks, hipStream_t stream, const pose_blend_launch& launch, const bounds_types&... bounds)
	{
		const auto kernel = blend_poses_kernel<kNumBuffers, kObjectSpace, bounds_types...>;
		// above the default limit of dynamic LDS the kernel has to be told
		if (shape.lds_bytes > 64 * 1024 - 128)
			ACLHIP_CHECK_HIP(context, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(k_consumer_lds_bytes)));
		hipLaunchKernelGGL(kernel, dim3(num_blocks), dim3((1u << shape.log2_instances_per_block) * k_wave_size), shape.lds_bytes, stream, launch, bounds...);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
		return ACLHIP_OK;
	}

	// (nine instantiations: K = 2, 3, 4 x local / object / object with bounds)
	template<uint32_t kNumBuffers>
	aclhip_status launch_blend_poses_of(aclhip_context* context, const consumer_launch_shape& shape, uint32_t num_blocks, hipStream_t stream, const pose_blend_launch& launch,
		bool object_space, const aclhip_pose_bounds* pose_bounds)
	{
		if (pose_bounds != nullptr)
			return launch_blend_poses_kernel<kNumBuffers, true>(context, shape, num_blocks, stream, launch, consumer_bounds_launch{ static_cast<uint8_t*>(pose_bounds->bounds), pose_bounds->bone_flags });
		return object_space ? launch_blend_poses_kernel<kNumBuffers, true>(context, shape, num_blocks, stream, launch)
			: launch_blend_poses_kernel<kNumBuffers, false>(context, shape, num_blocks, stream, launch);
	}

	// The launch: shaped by its rows alone, like launch_pose_buffers; the skeleton table and the mask table are filled in under the registry
	// lock (no mask registered yet: a table of no records -- every handle but the null handle is refused in the kernel); nothing is uploaded
	aclhip_status launch_pose_buffer_blend(aclhip_context* context, const aclhip_pose_buffer_blend& blend, uint32_t num_instances, void* poses, uint64_t pose_stride_bytes, hipStream_t stream)
	{
		std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
		if (context->skeletons.d_records == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no skeleton was ever registered with this context");
		const bool object_space = blend.object_space != 0;
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_buffer_launch_shape_of(context, poses, pose_stride_bytes, blend.buffer_stride_bytes[0], object_space, context->max_skeleton_hierarchy_words, shape); shape_status != ACLHIP_OK)
			return shape_status;
		note_launch_stream(context, stream);

		pose_blend_launch launch = {};
		launch.skeletons = context->skeletons.d_records;
		launch.num_skeletons = ACLHIP_MAX_SKELETONS;
		launch.skeleton = blend.skeleton;
		launch.instance_skeletons = blend.instance_skeletons;
		launch.masks = context->blend_masks.d_records;
		launch.num_masks = context->blend_masks.d_records != nullptr ? ACLHIP_MAX_BLEND_MASKS : 0u;
		launch.layered = blend.mode == ACLHIP_BLEND_LAYERED ? 1u : 0u;
		launch.instance_masks = blend.instance_masks;
		launch.weights = blend.weights;
		for (uint32_t k = 0; k < blend.num_buffers; ++k)
		{
			launch.buffers[k] = static_cast<const uint8_t*>(blend.buffers[k]);
			launch.buffer_stride_bytes[k] = blend.buffer_stride_bytes[k];
		}
		launch.poses = static_cast<uint8_t*>(poses);
		launch.pose_stride_bytes = pose_stride_bytes;
		launch.num_instances = num_instances;
		launch.lds_quads_per_image = shape.lds_quads_per_image;
		launch.lds_bytes_per_instance = uint32_t(shape.lds_bytes_per_instance);
		launch.packed_block_shape = shape.log2_instances_per_block | (shape.lds_schedule_words << 8);
		launch.rejected_count = context->d_rejected;

		const uint32_t instances_per_block = 1u << shape.log2_instances_per_block;
		const uint32_t num_blocks = (num_instances + instances_per_block - 1) / instances_per_block;
		switch (blend.num_buffers)
		{
		case 2: return launch_blend_poses_of<2>(context, shape, num_blocks, stream, launch, object_space, blend.bounds);
		case 3: return launch_blend_poses_of<3>(context, shape, num_blocks, stream, launch, object_space, blend.bounds);
		default: return launch_blend_poses_of<4>(context, shape, num_blocks, stream, launch, object_space, blend.bounds);
		}
	}

	// ---- object -> local space and make-additive (aclhip_inverse_transform_poses_batch; inverse_transform_poses_kernel) --------------------

	// What aclhip_inverse_transform_poses_batch checks of its arguments before any device call; every refusal leaves a message, with or without a context
	aclhip_status check_pose_buffer_inverse(aclhip_context* context, const void* source_poses, uint64_t source_pose_stride_bytes, uint32_t num_instances,
		const aclhip_pose_buffer_inverse* inverse, const void* poses, uint64_t pose_stride_bytes)
	{
		if (inverse == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose buffer inverse");
		if (source_poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null source pose buffer");
		if (poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null output buffer");
		if (inverse->skeleton == 0 && inverse->instance_skeletons == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a pose buffer inverse names a skeleton or a list of skeletons");
		if (inverse->additive_format > ACLHIP_ADDITIVE_ADDITIVE1)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown additive format %u", inverse->additive_format);
		const bool has_base = inverse->additive_format != ACLHIP_ADDITIVE_NONE;
		if (inverse->local_space == 0 && !has_base)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "neither local_space nor an additive format: nothing to do");
		if (has_base != (inverse->base_poses != nullptr))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "an additive format and a base pose buffer come together");
		if ((source_pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(source_poses) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "source pose buffer and stride must be 16 byte aligned");
		if ((pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(poses) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose buffer and stride must be 16 byte aligned");
		if (has_base && ((inverse->base_pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(inverse->base_poses) & 15u) != 0))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "base pose buffer and stride must be 16 byte aligned");
		if (inverse->reserved[0] != 0 || inverse->reserved[1] != 0 || inverse->reserved[2] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a pose buffer inverse are 0");
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_buffer_launch_shape_of(context, poses, pose_stride_bytes, source_pose_stride_bytes, false, 0, shape); shape_status != ACLHIP_OK)
			return shape_status;
		// in place is the one overlap allowed: a wave reads its own instance's row and has it complete in LDS before it stores
		const bool in_place = poses == source_poses && pose_stride_bytes == source_pose_stride_bytes;
		if (!in_place && pose_ranges_overlap(poses, pose_stride_bytes, source_poses, source_pose_stride_bytes, num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the output rows overlap the source pose rows: only poses == source_poses with equal strides (in place) is allowed");
		if (has_base && pose_ranges_overlap(poses, pose_stride_bytes, inverse->base_poses, inverse->base_pose_stride_bytes, num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the output rows overlap the base pose rows");
		return ACLHIP_OK;
	}

	template<bool kLocalSpace, bool kBase>
	aclhip_status launch_inverse_transform_poses_kernel(aclhip_context* context, const consumer_launch_shape& shape, uint32_t num_blocks, hipStream_t stream, const pose_inverse_launch& launch)
	{
		const auto kernel = inverse_transform_poses_kernel<kLocalSpace, kBase>;
		// above the default limit of dynamic LDS the kernel has to be told
		if (shape.lds_bytes > 64 * 1024 - 128)
			ACLHIP_CHECK_HIP(context, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(k_consumer_lds_bytes)));
		hipLaunchKernelGGL(kernel, dim3(num_blocks), dim3((1u << shape.log2_instances_per_block) * k_wave_size), shape.lds_bytes, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
		return ACLHIP_OK;
	}

	// The launch: shaped by its output rows alone, like launch_pose_buffers but without a walk schedule (the kernel has no walk); the skeleton
	// table is filled in under the registry lock; nothing is uploaded
	aclhip_status launch_pose_buffer_inverse(aclhip_context* context, const void* source_poses, uint64_t source_pose_stride_bytes, uint32_t num_instances,
		const aclhip_pose_buffer_inverse& inverse, void* poses, uint64_t pose_stride_bytes, hipStream_t stream)
	{
		std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
		if (context->skeletons.d_records == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no skeleton was ever registered with this context");
		const bool local_space = inverse.local_space != 0;
		const bool has_base = inverse.additive_format != ACLHIP_ADDITIVE_NONE;
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_buffer_launch_shape_of(context, poses, pose_stride_bytes, source_pose_stride_bytes, false, 0, shape); shape_status != ACLHIP_OK)
			return shape_status;
		note_launch_stream(context, stream);

		pose_inverse_launch launch = {};
		launch.skeletons = context->skeletons.d_records;
		launch.num_skeletons = ACLHIP_MAX_SKELETONS;
		launch.skeleton = inverse.skeleton;
		launch.instance_skeletons = inverse.instance_skeletons;
		launch.source_poses = static_cast<const uint8_t*>(source_poses);
		launch.source_pose_stride_bytes = source_pose_stride_bytes;
		launch.base_poses = has_base ? static_cast<const uint8_t*>(inverse.base_poses) : nullptr;
		launch.base_pose_stride_bytes = has_base ? inverse.base_pose_stride_bytes : 0;
		launch.poses = static_cast<uint8_t*>(poses);
		launch.pose_stride_bytes = pose_stride_bytes;
		launch.num_instances = num_instances;
		launch.additive_format = inverse.additive_format;
		launch.lds_quads_per_image = shape.lds_quads_per_image;
		launch.lds_bytes_per_instance = uint32_t(shape.lds_bytes_per_instance);
		launch.log2_instances_per_block = shape.log2_instances_per_block;
		launch.rejected_count = context->d_rejected;

		const uint32_t instances_per_block = 1u << shape.log2_instances_per_block;
		const uint32_t num_blocks = (num_instances + instances_per_block - 1) / instances_per_block;
		// three instantiations: local / none, local / base, no-local / base
		if (!local_space)
			return launch_inverse_transform_poses_kernel<false, true>(context, shape, num_blocks, stream, launch);
		return has_base ? launch_inverse_transform_poses_kernel<true, true>(context, shape, num_blocks, stream, launch)
			: launch_inverse_transform_poses_kernel<true, false>(context, shape, num_blocks, stream, launch);
	}

	// ---- the shell error of two pose buffers (aclhip_measure_pose_error_batch; measure_pose_error_kernel) ---------------------------------

	// The two input rows set the shape of the launch: an image's quads from the smaller stride, two images per instance, and the words of the
	// walk schedule on top of them once the context is known. Refuses rows that do not fit.
	aclhip_status pose_error_launch_shape_of(aclhip_context* context, uint64_t raw_pose_stride_bytes, uint64_t lossy_pose_stride_bytes, bool object_space,
		uint32_t max_hierarchy_words, consumer_launch_shape& out_shape)
	{
		const uint32_t row_transforms = uint32_t(std::min<uint64_t>(std::min(raw_pose_stride_bytes, lossy_pose_stride_bytes) / 48, 0xFFFFu));
		out_shape = consumer_launch_shape_of(row_transforms * 3u, row_transforms, true, object_space, max_hierarchy_words);
		if (!out_shape.fits)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "rows of %u transforms: two of them are too large for the pose error measure (%zu bytes of LDS per instance)", row_transforms, out_shape.lds_needed_bytes);
		return ACLHIP_OK;
	}

	// What aclhip_measure_pose_error_batch checks of its arguments before any device call; every refusal leaves a message, with or without a context
	aclhip_status check_pose_error(aclhip_context* context, const void* raw_poses, uint64_t raw_pose_stride_bytes, const void* lossy_poses, uint64_t lossy_pose_stride_bytes,
		uint32_t num_instances, const aclhip_pose_error_desc* desc, const aclhip_pose_error* errors)
	{
		if (desc == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose error desc");
		if (raw_poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null raw pose buffer");
		if (lossy_poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null lossy pose buffer");
		if (errors == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose error records");
		if (desc->skeleton == 0 && desc->instance_skeletons == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a pose error desc names a skeleton or a list of skeletons");
		if (desc->additive_format > ACLHIP_ADDITIVE_ADDITIVE1)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown additive format %u", desc->additive_format);
		const bool has_base = desc->additive_format != ACLHIP_ADDITIVE_NONE;
		if (has_base != (desc->base_poses != nullptr))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "an additive format and a base pose buffer come together");
		if (desc->shell_distances != nullptr && desc->num_shell_distances == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a shell distance table of no entries");
		if (desc->bone_errors != nullptr && (desc->bone_error_stride_bytes == 0 || (desc->bone_error_stride_bytes & 3u) != 0 || (reinterpret_cast<uintptr_t>(desc->bone_errors) & 3u) != 0))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "bone errors are 4 byte aligned and their stride is a multiple of 4 that is not 0");
		if ((raw_pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(raw_poses) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "raw pose buffer and stride must be 16 byte aligned");
		if ((lossy_pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(lossy_poses) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "lossy pose buffer and stride must be 16 byte aligned");
		if (has_base && ((desc->base_pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(desc->base_poses) & 15u) != 0))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "base pose buffer and stride must be 16 byte aligned");
		if ((reinterpret_cast<uintptr_t>(errors) & 7u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose error records must be 8 byte aligned");
		if ((reinterpret_cast<uintptr_t>(desc->worst) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the worst pose error record must be 16 byte aligned");
		if (desc->reserved[0] != 0 || desc->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a pose error desc are 0");
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_error_launch_shape_of(context, raw_pose_stride_bytes, lossy_pose_stride_bytes, false, 0, shape); shape_status != ACLHIP_OK)
			return shape_status;

		// raw, lossy and base are only read and may overlap each other freely; what is written overlaps nothing that is read and no other output
		const unsigned __int128 n = num_instances;
		return check_no_overlap(context,
			{
				{ "the pose error records", errors, n * sizeof(aclhip_pose_error) },
				{ "the bone errors", desc->bone_errors, desc->bone_errors != nullptr ? n * desc->bone_error_stride_bytes : 0 },
				{ "the worst record", desc->worst, desc->worst != nullptr ? sizeof(aclhip_pose_error_worst) : 0 },
			},
			{
				{ "the raw pose rows", raw_poses, n * raw_pose_stride_bytes }, { "the lossy pose rows", lossy_poses, n * lossy_pose_stride_bytes },
				{ "the base pose rows", desc->base_poses, has_base ? n * desc->base_pose_stride_bytes : 0 },
				{ "the skeleton list", desc->instance_skeletons, desc->instance_skeletons != nullptr ? n * sizeof(aclhip_skeleton) : 0 },
				{ "the shell distances", desc->shell_distances, desc->shell_distances != nullptr ? (unsigned __int128)desc->num_shell_distances * sizeof(float) : 0 },
			});
	}

	template<class kernel_type>
	aclhip_status launch_measure_pose_error_kernel(aclhip_context* context, kernel_type kernel, const consumer_launch_shape& shape, uint32_t num_blocks, hipStream_t stream, const pose_error_launch& launch)
	{
		// above the default limit of dynamic LDS the kernel has to be told
		if (shape.lds_bytes > 64 * 1024 - 128)
			ACLHIP_CHECK_HIP(context, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(k_consumer_lds_bytes)));
		// two waves per instance: one per image
		hipLaunchKernelGGL(kernel, dim3(num_blocks), dim3((2u << shape.log2_instances_per_block) * k_wave_size), shape.lds_bytes, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
		return ACLHIP_OK;
	}

	// The launch: shaped by its two input rows alone; the skeleton table is filled in under the registry lock; nothing is uploaded. The
	// worst record is a second, one workgroup launch over the instances' records on the same stream -- the only launch of a batch of none.
	aclhip_status launch_pose_error(aclhip_context* context, const void* raw_poses, uint64_t raw_pose_stride_bytes, const void* lossy_poses, uint64_t lossy_pose_stride_bytes,
		uint32_t num_instances, const aclhip_pose_error_desc& desc, uint32_t metric, aclhip_pose_error* errors, hipStream_t stream)
	{
		std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
		if (num_instances != 0)
		{
			if (context->skeletons.d_records == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no skeleton was ever registered with this context");
			const bool object_space = desc.object_space != 0;
			const bool has_base = desc.additive_format != ACLHIP_ADDITIVE_NONE;
			consumer_launch_shape shape;
			if (const aclhip_status shape_status = pose_error_launch_shape_of(context, raw_pose_stride_bytes, lossy_pose_stride_bytes, object_space, context->max_skeleton_hierarchy_words, shape); shape_status != ACLHIP_OK)
				return shape_status;
			note_launch_stream(context, stream);

			pose_error_launch launch = {};
			launch.skeletons = context->skeletons.d_records;
			launch.num_skeletons = ACLHIP_MAX_SKELETONS;
			launch.skeleton = desc.skeleton;
			launch.instance_skeletons = desc.instance_skeletons;
			launch.raw_poses = static_cast<const uint8_t*>(raw_poses);
			launch.raw_pose_stride_bytes = raw_pose_stride_bytes;
			launch.lossy_poses = static_cast<const uint8_t*>(lossy_poses);
			launch.lossy_pose_stride_bytes = lossy_pose_stride_bytes;
			launch.base_poses = has_base ? static_cast<const uint8_t*>(desc.base_poses) : nullptr;
			launch.base_pose_stride_bytes = has_base ? desc.base_pose_stride_bytes : 0;
			launch.shell_distances = desc.shell_distances;
			launch.num_shell_distances = desc.num_shell_distances;
			launch.shell_distance = desc.shell_distance;
			launch.bone_errors = reinterpret_cast<uint8_t*>(desc.bone_errors);
			launch.bone_error_stride_bytes = desc.bone_error_stride_bytes;
			launch.errors = reinterpret_cast<pose_error_record*>(errors);
			launch.num_instances = num_instances;
			launch.additive_format = desc.additive_format;
			launch.lds_quads_per_image = shape.lds_quads_per_image;
			launch.lds_bytes_per_instance = uint32_t(shape.lds_bytes_per_instance);
			launch.packed_block_shape = shape.log2_instances_per_block | (shape.lds_schedule_words << 8);
			launch.rejected_count = context->d_rejected;

			const uint32_t instances_per_block = 1u << shape.log2_instances_per_block;
			const uint32_t num_blocks = (num_instances + instances_per_block - 1) / instances_per_block;
			// four instantiations: object / local x base / none, and the matrix metric's two: object / local (it takes no base)
			const auto kernel = metric == ACLHIP_METRIC_QVVF_MATRIX3X4F
				? (object_space ? measure_pose_error_kernel<true, false, true> : measure_pose_error_kernel<false, false, true>)
				: object_space ? (has_base ? measure_pose_error_kernel<true, true, false> : measure_pose_error_kernel<true, false, false>)
				: (has_base ? measure_pose_error_kernel<false, true, false> : measure_pose_error_kernel<false, false, false>);
			const aclhip_status status = launch_measure_pose_error_kernel(context, kernel, shape, num_blocks, stream, launch);
			if (status != ACLHIP_OK)
				return status;
		}
		else
			note_launch_stream(context, stream);
		if (desc.worst != nullptr)
		{
			hipLaunchKernelGGL(pose_error_worst_kernel, dim3(1), dim3(k_pose_error_worst_threads), 0, stream, reinterpret_cast<const pose_error_record*>(errors), num_instances,
				reinterpret_cast<u32x4*>(desc.worst));
			ACLHIP_CHECK_HIP(context, hipGetLastError());
		}
		return ACLHIP_OK;
	}

	// ---- 3x4 matrices of a pose buffer (aclhip_pose_matrices_batch; pose_matrices_kernel) -------------------------------------------------

	// Both rows set the shape of the launch: an image holds min(local_pose_stride_bytes / 48, matrix_stride_bytes / 64) transforms (a
	// matrix takes the three quads of its QVV record), and the words of the walk schedule on top once the context is known
	aclhip_status pose_matrices_launch_shape_of(aclhip_context* context, uint64_t local_pose_stride_bytes, uint64_t matrix_stride_bytes, bool object_space,
		uint32_t max_hierarchy_words, consumer_launch_shape& out_shape)
	{
		const uint32_t row_transforms = uint32_t(std::min<uint64_t>(std::min(local_pose_stride_bytes / 48, matrix_stride_bytes / 64), 0xFFFFu));
		out_shape = consumer_launch_shape_of(row_transforms * 3u, row_transforms, false, object_space, max_hierarchy_words);
		if (!out_shape.fits)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "rows of %u transforms: too large for the pose matrices (%zu bytes of LDS per instance)", row_transforms, out_shape.lds_needed_bytes);
		return ACLHIP_OK;
	}

	// What aclhip_pose_matrices_batch checks of its arguments before any device call; every refusal leaves a message, with or without a context
	aclhip_status check_pose_matrices(aclhip_context* context, const void* local_poses, uint64_t local_pose_stride_bytes, uint32_t num_instances,
		const aclhip_pose_matrices_desc* desc, const void* matrices, uint64_t matrix_stride_bytes)
	{
		if (desc == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose matrices desc");
		if (local_poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null local pose buffer");
		if (matrices == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null matrix buffer");
		if (desc->skeleton == 0 && desc->instance_skeletons == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a pose matrices desc names a skeleton or a list of skeletons");
		if (desc->layout != ACLHIP_MATRIX_3X4F_64)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown matrix layout %u", desc->layout);
		if ((local_pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(local_poses) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "local pose buffer and stride must be 16 byte aligned");
		if ((matrix_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(matrices) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "matrix buffer and stride must be 16 byte aligned");
		if (desc->reserved[0] != 0 || desc->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a pose matrices desc are 0");
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_matrices_launch_shape_of(context, local_pose_stride_bytes, matrix_stride_bytes, false, 0, shape); shape_status != ACLHIP_OK)
			return shape_status;
		// records differ in size: there is no in place form, and no other overlap either (the skeleton list is only read as well)
		if (pose_ranges_overlap(matrices, matrix_stride_bytes, local_poses, local_pose_stride_bytes, num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the matrix rows overlap the local pose rows: a matrix is larger than its transform, there is no in place form");
		if (desc->instance_skeletons != nullptr && pose_ranges_overlap(matrices, matrix_stride_bytes, desc->instance_skeletons, sizeof(aclhip_skeleton), num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the matrix rows overlap the skeleton list");
		return ACLHIP_OK;
	}

	template<bool kObjectSpace>
	aclhip_status launch_pose_matrices_kernel(aclhip_context* context, const consumer_launch_shape& shape, uint32_t num_blocks, hipStream_t stream, const pose_matrices_launch& launch)
	{
		const auto kernel = pose_matrices_kernel<kObjectSpace>;
		// above the default limit of dynamic LDS the kernel has to be told
		if (shape.lds_bytes > 64 * 1024 - 128)
			ACLHIP_CHECK_HIP(context, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(k_consumer_lds_bytes)));
		hipLaunchKernelGGL(kernel, dim3(num_blocks), dim3((1u << shape.log2_instances_per_block) * k_wave_size), shape.lds_bytes, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
		return ACLHIP_OK;
	}

	// The launch: shaped by its rows alone, like launch_pose_buffers; the skeleton table is filled in under the registry lock; nothing is uploaded
	aclhip_status launch_pose_matrices(aclhip_context* context, const void* local_poses, uint64_t local_pose_stride_bytes, uint32_t num_instances,
		const aclhip_pose_matrices_desc& desc, void* matrices, uint64_t matrix_stride_bytes, hipStream_t stream)
	{
		std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
		if (context->skeletons.d_records == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no skeleton was ever registered with this context");
		const bool object_space = desc.object_space != 0;
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_matrices_launch_shape_of(context, local_pose_stride_bytes, matrix_stride_bytes, object_space, context->max_skeleton_hierarchy_words, shape); shape_status != ACLHIP_OK)
			return shape_status;
		note_launch_stream(context, stream);

		pose_matrices_launch launch = {};
		launch.skeletons = context->skeletons.d_records;
		launch.num_skeletons = ACLHIP_MAX_SKELETONS;
		launch.skeleton = desc.skeleton;
		launch.instance_skeletons = desc.instance_skeletons;
		launch.local_poses = static_cast<const uint8_t*>(local_poses);
		launch.local_pose_stride_bytes = local_pose_stride_bytes;
		launch.matrices = static_cast<uint8_t*>(matrices);
		launch.matrix_stride_bytes = matrix_stride_bytes;
		launch.num_instances = num_instances;
		launch.lds_quads_per_image = shape.lds_quads_per_image;
		launch.lds_bytes_per_instance = uint32_t(shape.lds_bytes_per_instance);
		launch.packed_block_shape = shape.log2_instances_per_block | (shape.lds_schedule_words << 8);
		launch.rejected_count = context->d_rejected;

		const uint32_t instances_per_block = 1u << shape.log2_instances_per_block;
		const uint32_t num_blocks = (num_instances + instances_per_block - 1) / instances_per_block;
		return object_space ? launch_pose_matrices_kernel<true>(context, shape, num_blocks, stream, launch) : launch_pose_matrices_kernel<false>(context, shape, num_blocks, stream, launch);
	}
}

// include/aclhip.h states the definition. The argument checks need no device, come first and leave a message, with or without a context.
extern "C" aclhip_status aclhip_transform_poses_batch(aclhip_context* context, const void* local_poses, uint64_t local_pose_stride_bytes, uint32_t num_instances,
	const aclhip_pose_buffer_consumers* consumers, void* poses, uint64_t pose_stride_bytes, void* stream)
{
	const aclhip_status status = check_pose_buffer_consumers(context, local_poses, local_pose_stride_bytes, num_instances, consumers, poses, pose_stride_bytes);
	if (status != ACLHIP_OK)
		return status;
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	if (num_instances == 0)
		return ACLHIP_OK;

	device_guard guard(context->device);
	return launch_pose_buffers(context, local_poses, local_pose_stride_bytes, num_instances, *consumers, poses, pose_stride_bytes, static_cast<hipStream_t>(stream));
}

// include/aclhip.h states the definition. The argument checks need no device, come first and leave a message, with or without a context.
extern "C" aclhip_status aclhip_blend_poses_batch(aclhip_context* context, const aclhip_pose_buffer_blend* blend, uint32_t num_instances, void* poses, uint64_t pose_stride_bytes, void* stream)
{
	const aclhip_status status = check_pose_buffer_blend(context, blend, num_instances, poses, pose_stride_bytes);
	if (status != ACLHIP_OK)
		return status;
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	if (num_instances == 0)
		return ACLHIP_OK;

	device_guard guard(context->device);
	return launch_pose_buffer_blend(context, *blend, num_instances, poses, pose_stride_bytes, static_cast<hipStream_t>(stream));
}

// include/aclhip.h states the definition. The argument checks need no device, come first and leave a message, with or without a context.
extern "C" aclhip_status aclhip_inverse_transform_poses_batch(aclhip_context* context, const void* source_poses, uint64_t source_pose_stride_bytes, uint32_t num_instances,
	const aclhip_pose_buffer_inverse* inverse, void* poses, uint64_t pose_stride_bytes, void* stream)
{
	const aclhip_status status = check_pose_buffer_inverse(context, source_poses, source_pose_stride_bytes, num_instances, inverse, poses, pose_stride_bytes);
	if (status != ACLHIP_OK)
		return status;
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	if (num_instances == 0)
		return ACLHIP_OK;

	device_guard guard(context->device);
	return launch_pose_buffer_inverse(context, source_poses, source_pose_stride_bytes, num_instances, *inverse, poses, pose_stride_bytes, static_cast<hipStream_t>(stream));
}

// include/aclhip.h states the definition. The argument checks need no device, come first and leave a message, with or without a context.
extern "C" aclhip_status aclhip_measure_pose_error_metric_batch(aclhip_context* context, const void* raw_poses, uint64_t raw_pose_stride_bytes, const void* lossy_poses,
	uint64_t lossy_pose_stride_bytes, uint32_t num_instances, const aclhip_pose_error_desc* desc, uint32_t metric, aclhip_pose_error* errors, void* stream)
{
	const aclhip_status status = check_pose_error(context, raw_poses, raw_pose_stride_bytes, lossy_poses, lossy_pose_stride_bytes, num_instances, desc, errors);
	if (status != ACLHIP_OK)
		return status;
	if (metric > ACLHIP_METRIC_QVVF_MATRIX3X4F)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown error metric %u", metric);
	if (metric == ACLHIP_METRIC_QVVF_MATRIX3X4F && desc->additive_format != ACLHIP_ADDITIVE_NONE)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the matrix error metric takes no additive format: apply_additive_to_base is defined over QVV poses only");
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	// (a batch of no instances still writes the launch's worst record)
	if (num_instances == 0 && desc->worst == nullptr)
		return ACLHIP_OK;

	device_guard guard(context->device);
	return launch_pose_error(context, raw_poses, raw_pose_stride_bytes, lossy_poses, lossy_pose_stride_bytes, num_instances, *desc, metric, errors, static_cast<hipStream_t>(stream));
}

// ACLHIP_METRIC_QVVF of the call above: one host path
extern "C" aclhip_status aclhip_measure_pose_error_batch(aclhip_context* context, const void* raw_poses, uint64_t raw_pose_stride_bytes, const void* lossy_poses,
	uint64_t lossy_pose_stride_bytes, uint32_t num_instances, const aclhip_pose_error_desc* desc, aclhip_pose_error* errors, void* stream)
{
	return aclhip_measure_pose_error_metric_batch(context, raw_poses, raw_pose_stride_bytes, lossy_poses, lossy_pose_stride_bytes, num_instances, desc, ACLHIP_METRIC_QVVF, errors, stream);
}

// include/aclhip.h states the definition. The argument checks need no device, come first and leave a message, with or without a context.
extern "C" aclhip_status aclhip_pose_matrices_batch(aclhip_context* context, const void* local_poses, uint64_t local_pose_stride_bytes, uint32_t num_instances,
	const aclhip_pose_matrices_desc* desc, void* matrices, uint64_t matrix_stride_bytes, void* stream)
{
	const aclhip_status status = check_pose_matrices(context, local_poses, local_pose_stride_bytes, num_instances, desc, matrices, matrix_stride_bytes);
	if (status != ACLHIP_OK)
		return status;
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	if (num_instances == 0)
		return ACLHIP_OK;

	device_guard guard(context->device);
	return launch_pose_matrices(context, local_poses, local_pose_stride_bytes, num_instances, *desc, matrices, matrix_stride_bytes, static_cast<hipStream_t>(stream));
}
