// host_pose_buffers.inl -- part of aclhip.hip (one translation unit; included there, in this order, not compiled on its own).
// Host side: the pose consumers over a caller's pose buffers (aclhip_transform_poses_batch, aclhip_blend_poses_batch,
// aclhip_inverse_transform_poses_batch, aclhip_measure_pose_error_batch and its _metric form, aclhip_pose_matrices_batch;
// kernels_pose_buffers.inl). What the launches over a caller's pose rows do alike stands first -- the clauses their argument checks
// share, the shape of rows, the front behind the checks and the common fields of the kernels' arguments; host_skins.inl, behind this
// file, uses them for aclhip_skinning_matrices_batch. Each entry point keeps what is its own: the order of its checks, its rule for
// the rows, its kernel's argument and the choice of the instantiation.

namespace
{
	// ---- what the launches over a caller's pose rows do alike -----------------------------------------------------------------------------

	// The clauses of the argument checks that come back in every one of them; an entry point calls them where its own order has them.
	// Rows are 16 byte aligned, the buffer and the stride: the first of `buffers` that is not (a null buffer with a stride of 0 is)
	struct named_rows { const char* name; const void* rows; uint64_t stride_bytes; };
	aclhip_status check_rows_aligned(const aclhip_context* context, std::initializer_list<named_rows> buffers)
	{
		for (const named_rows& buffer : buffers)
			if ((buffer.stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(buffer.rows) & 15u) != 0)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s buffer and stride must be 16 byte aligned", buffer.name);
		return ACLHIP_OK;
	}

	// `subject`: "a pose matrices desc names"
	aclhip_status check_names_skeleton(const aclhip_context* context, const char* subject, aclhip_skeleton skeleton, const aclhip_skeleton* instance_skeletons)
	{
		if (skeleton == 0 && instance_skeletons == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s a skeleton or a list of skeletons", subject);
		return ACLHIP_OK;
	}

	aclhip_status check_additive_format(const aclhip_context* context, uint32_t additive_format)
	{
		if (additive_format > ACLHIP_ADDITIVE_ADDITIVE1)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown additive format %u", additive_format);
		return ACLHIP_OK;
	}

	// `buffer_name`: "a base pose buffer", the rows the format combines with
	aclhip_status check_format_with_buffer(const aclhip_context* context, uint32_t additive_format, const void* buffer, const char* buffer_name)
	{
		if ((additive_format != ACLHIP_ADDITIVE_NONE) != (buffer != nullptr))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "an additive format and %s come together", buffer_name);
		return ACLHIP_OK;
	}

	// The rows that set the shape of a launch, by the entry point's own rule (its check states it): the transforms an image holds, one
	// image per instance or two, and what the refusal says of rows that do not fit
	struct pose_rows { uint64_t transforms; bool two_waves; const char* too_large; };

	// The rows alone set the shape of the launch: an image's quads, and the words of the walk schedule on top of them once the context is
	// known (launch_pose_rows; the argument checks ask without them: not in object space, no words). Refuses rows that do not fit.
	aclhip_status pose_rows_launch_shape_of(const aclhip_context* context, const pose_rows& rows, bool object_space, uint32_t max_hierarchy_words, consumer_launch_shape& out_shape)
	{
		const uint32_t row_transforms = uint32_t(std::min<uint64_t>(rows.transforms, 0xFFFFu));
		out_shape = consumer_launch_shape_of(row_transforms * 3u, row_transforms, rows.two_waves, object_space, max_hierarchy_words);
		if (!out_shape.fits)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "rows of %u transforms: %s (%zu bytes of LDS per instance)", row_transforms, rows.too_large, out_shape.lds_needed_bytes);
		return ACLHIP_OK;
	}

	// The front of the entry points behind their checks (launch_compress's, host_scalar_compress.inl, for a caller's pose rows): the null
	// context, the batch of none, the device, the registry lock (shared: see launch_tracks), the tables the launch names -- the skeletons,
	// and the skins when it `names_skin` --, the shape with the context's longest walk schedule, the stream. `launch(stream, shape, num_blocks)`
	// fills in its kernel's argument and picks the instantiation; launches are shaped by their rows alone, like the mapped launch
	// (registered clips play no part), and nothing is uploaded. `runs_batch_of_none`: a batch of no instances has something to launch
	// all the same (the pose error measure's worst record); it names no table and has no shape: its launch is handed no block.
	template<class launch_function>
	aclhip_status launch_pose_rows(aclhip_context* context, uint32_t num_instances, void* stream_handle, const pose_rows& rows, bool object_space, bool names_skin,
		bool runs_batch_of_none, launch_function launch)
	{
		if (context == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
		if (num_instances == 0 && !runs_batch_of_none)
			return ACLHIP_OK;

		device_guard guard(context->device);
		hipStream_t stream = static_cast<hipStream_t>(stream_handle);
		std::shared_lock<std::shared_mutex> lock(context->mutex);
		consumer_launch_shape shape = {};
		if (num_instances != 0)
		{
			if (context->skeletons.d_records == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no skeleton was ever registered with this context");
			if (names_skin && context->skins.d_records == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no skin was ever registered with this context");
			if (const aclhip_status status = pose_rows_launch_shape_of(context, rows, object_space, context->max_skeleton_hierarchy_words, shape); status != ACLHIP_OK)
				return status;
		}
		note_launch_stream(context, stream);
		const uint32_t instances_per_block = 1u << shape.log2_instances_per_block;
		return launch(stream, shape, (num_instances + instances_per_block - 1) / instances_per_block);
	}

	// The two ends every kernel's argument has (kernels_pose_buffers.inl): the skeleton table and the skeletons the entry point's struct
	// names, and the instances with the images of the shape. The rows between them are the caller's.
	pose_rows_head pose_rows_head_of(const aclhip_context* context, aclhip_skeleton skeleton, const aclhip_skeleton* instance_skeletons)
	{
		return { context->skeletons.d_records, ACLHIP_MAX_SKELETONS, skeleton, instance_skeletons };
	}

	pose_rows_shape pose_rows_shape_of(const aclhip_context* context, uint32_t num_instances, const consumer_launch_shape& shape)
	{
		return { num_instances, shape.lds_quads_per_image, uint32_t(shape.lds_bytes_per_instance), shape.log2_instances_per_block | (shape.lds_schedule_words << 8), context->d_rejected };
	}

	// ---- object space and additive apply (aclhip_transform_poses_batch; transform_poses_kernel) --------------------------------------------

	// What aclhip_transform_poses_batch checks of its arguments before any device call; every refusal leaves a message, with or without a
	// context. The rows that shape the launch: the output rows when there are any, else the local rows.
	aclhip_status check_pose_buffer_consumers(aclhip_context* context, const void* local_poses, uint64_t local_pose_stride_bytes, uint32_t num_instances,
		const aclhip_pose_buffer_consumers* consumers, const void* poses, uint64_t pose_stride_bytes, pose_rows& out_rows)
	{
		if (consumers == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose buffer consumers");
		if (local_poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null local pose buffer");
		if (const aclhip_status status = check_names_skeleton(context, "pose buffer consumers name", consumers->skeleton, consumers->instance_skeletons); status != ACLHIP_OK)
			return status;
		if (const aclhip_status status = check_additive_format(context, consumers->additive_format); status != ACLHIP_OK)
			return status;
		const bool has_additive = consumers->additive_format != ACLHIP_ADDITIVE_NONE;
		if (consumers->object_space == 0 && !has_additive)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "neither object_space nor an additive format: nothing to do");
		if (const aclhip_status status = check_format_with_buffer(context, consumers->additive_format, consumers->additive_poses, "an additive pose buffer"); status != ACLHIP_OK)
			return status;
		if (consumers->bounds != nullptr && consumers->object_space == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose bounds are taken in object space: a local space translation is not a position");
		if (poses == nullptr && consumers->bounds == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null output buffer without bounds");
		if (const aclhip_status status = check_rows_aligned(context, { { "local pose", local_poses, local_pose_stride_bytes }, { "pose", poses, pose_stride_bytes },
				{ "additive pose", consumers->additive_poses, has_additive ? consumers->additive_pose_stride_bytes : 0 } }); status != ACLHIP_OK)
			return status;
		if (consumers->reserved[0] != 0 || consumers->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of pose buffer consumers are 0");
		if (consumers->bounds != nullptr)
			if (const aclhip_status bounds_status = check_pose_bounds(context, consumers->bounds); bounds_status != ACLHIP_OK)
				return bounds_status;
		out_rows = { (poses != nullptr ? pose_stride_bytes : local_pose_stride_bytes) / 48, false, "too large for the pose consumers" };
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_rows_launch_shape_of(context, out_rows, false, 0, shape); shape_status != ACLHIP_OK)
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

	// ---- a blend of K caller pose buffers (aclhip_blend_poses_batch; blend_poses_kernel in kernels_pose_buffers.inl) ----------------------

	// What aclhip_blend_poses_batch checks of its arguments before any device call; every refusal leaves a message, with or without a
	// context. The rows that shape the launch: the output rows when there are any, else the rows of the first buffer.
	aclhip_status check_pose_buffer_blend(aclhip_context* context, const aclhip_pose_buffer_blend* blend, uint32_t num_instances, const void* poses, uint64_t pose_stride_bytes,
		pose_rows& out_rows)
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
		if (const aclhip_status status = check_names_skeleton(context, "a pose buffer blend names", blend->skeleton, blend->instance_skeletons); status != ACLHIP_OK)
			return status;
		if (blend->bounds != nullptr && blend->object_space == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose bounds are taken in object space: a local space translation is not a position");
		if (poses == nullptr && blend->bounds == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null output buffer without bounds");
		for (uint32_t k = 0; k < num_buffers; ++k)
			if ((blend->buffer_stride_bytes[k] & 15u) != 0 || (reinterpret_cast<uintptr_t>(blend->buffers[k]) & 15u) != 0)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose buffer %u and its stride must be 16 byte aligned", k);
		if (const aclhip_status status = check_rows_aligned(context, { { "pose", poses, pose_stride_bytes } }); status != ACLHIP_OK)
			return status;
		if (blend->reserved0 != 0 || blend->reserved[0] != 0 || blend->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a pose buffer blend are 0");
		if (blend->bounds != nullptr)
			if (const aclhip_status bounds_status = check_pose_bounds(context, blend->bounds); bounds_status != ACLHIP_OK)
				return bounds_status;
		out_rows = { (poses != nullptr ? pose_stride_bytes : blend->buffer_stride_bytes[0]) / 48, false, "too large for the pose consumers" };
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_rows_launch_shape_of(context, out_rows, false, 0, shape); shape_status != ACLHIP_OK)
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

	// (nine instantiations: K = 2, 3, 4 x local / object / object with bounds)
	template<uint32_t kNumBuffers>
	aclhip_status launch_blend_poses_of(aclhip_context* context, const consumer_launch_shape& shape, uint32_t num_blocks, hipStream_t stream, const pose_blend_launch& launch,
		bool object_space, const aclhip_pose_bounds* pose_bounds)
	{
		if (pose_bounds != nullptr)
			return launch_consumer_kernel(context, blend_poses_kernel<kNumBuffers, true, consumer_bounds_launch>, shape, num_blocks, 1, stream, launch,
				consumer_bounds_launch{ static_cast<uint8_t*>(pose_bounds->bounds), pose_bounds->bone_flags });
		return launch_consumer_kernel(context, object_space ? blend_poses_kernel<kNumBuffers, true> : blend_poses_kernel<kNumBuffers, false>, shape, num_blocks, 1, stream, launch);
	}

	// ---- object -> local space and make-additive (aclhip_inverse_transform_poses_batch; inverse_transform_poses_kernel) --------------------

	// What aclhip_inverse_transform_poses_batch checks of its arguments before any device call; every refusal leaves a message, with or
	// without a context. The rows that shape the launch: the output rows.
	aclhip_status check_pose_buffer_inverse(aclhip_context* context, const void* source_poses, uint64_t source_pose_stride_bytes, uint32_t num_instances,
		const aclhip_pose_buffer_inverse* inverse, const void* poses, uint64_t pose_stride_bytes, pose_rows& out_rows)
	{
		if (inverse == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose buffer inverse");
		if (source_poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null source pose buffer");
		if (poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null output buffer");
		if (const aclhip_status status = check_names_skeleton(context, "a pose buffer inverse names", inverse->skeleton, inverse->instance_skeletons); status != ACLHIP_OK)
			return status;
		if (const aclhip_status status = check_additive_format(context, inverse->additive_format); status != ACLHIP_OK)
			return status;
		const bool has_base = inverse->additive_format != ACLHIP_ADDITIVE_NONE;
		if (inverse->local_space == 0 && !has_base)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "neither local_space nor an additive format: nothing to do");
		if (const aclhip_status status = check_format_with_buffer(context, inverse->additive_format, inverse->base_poses, "a base pose buffer"); status != ACLHIP_OK)
			return status;
		if (const aclhip_status status = check_rows_aligned(context, { { "source pose", source_poses, source_pose_stride_bytes }, { "pose", poses, pose_stride_bytes },
				{ "base pose", inverse->base_poses, has_base ? inverse->base_pose_stride_bytes : 0 } }); status != ACLHIP_OK)
			return status;
		if (inverse->reserved[0] != 0 || inverse->reserved[1] != 0 || inverse->reserved[2] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a pose buffer inverse are 0");
		out_rows = { pose_stride_bytes / 48, false, "too large for the pose consumers" };
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_rows_launch_shape_of(context, out_rows, false, 0, shape); shape_status != ACLHIP_OK)
			return shape_status;
		// in place is the one overlap allowed: a wave reads its own instance's row and has it complete in LDS before it stores
		const bool in_place = poses == source_poses && pose_stride_bytes == source_pose_stride_bytes;
		if (!in_place && pose_ranges_overlap(poses, pose_stride_bytes, source_poses, source_pose_stride_bytes, num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the output rows overlap the source pose rows: only poses == source_poses with equal strides (in place) is allowed");
		if (has_base && pose_ranges_overlap(poses, pose_stride_bytes, inverse->base_poses, inverse->base_pose_stride_bytes, num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the output rows overlap the base pose rows");
		return ACLHIP_OK;
	}

	// ---- the shell error of two pose buffers (aclhip_measure_pose_error_batch; measure_pose_error_kernel) ---------------------------------

	// What aclhip_measure_pose_error_batch checks of its arguments before any device call; every refusal leaves a message, with or without
	// a context. The rows that shape the launch: both input rows -- an image's quads from the smaller stride, two images per instance.
	aclhip_status check_pose_error(aclhip_context* context, const void* raw_poses, uint64_t raw_pose_stride_bytes, const void* lossy_poses, uint64_t lossy_pose_stride_bytes,
		uint32_t num_instances, const aclhip_pose_error_desc* desc, const aclhip_pose_error* errors, pose_rows& out_rows)
	{
		if (desc == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose error desc");
		if (raw_poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null raw pose buffer");
		if (lossy_poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null lossy pose buffer");
		if (errors == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose error records");
		if (const aclhip_status status = check_names_skeleton(context, "a pose error desc names", desc->skeleton, desc->instance_skeletons); status != ACLHIP_OK)
			return status;
		if (const aclhip_status status = check_additive_format(context, desc->additive_format); status != ACLHIP_OK)
			return status;
		if (const aclhip_status status = check_format_with_buffer(context, desc->additive_format, desc->base_poses, "a base pose buffer"); status != ACLHIP_OK)
			return status;
		const bool has_base = desc->additive_format != ACLHIP_ADDITIVE_NONE;
		if (desc->shell_distances != nullptr && desc->num_shell_distances == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a shell distance table of no entries");
		if (desc->bone_errors != nullptr && (desc->bone_error_stride_bytes == 0 || (desc->bone_error_stride_bytes & 3u) != 0 || (reinterpret_cast<uintptr_t>(desc->bone_errors) & 3u) != 0))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "bone errors are 4 byte aligned and their stride is a multiple of 4 that is not 0");
		if (const aclhip_status status = check_rows_aligned(context, { { "raw pose", raw_poses, raw_pose_stride_bytes }, { "lossy pose", lossy_poses, lossy_pose_stride_bytes },
				{ "base pose", desc->base_poses, has_base ? desc->base_pose_stride_bytes : 0 } }); status != ACLHIP_OK)
			return status;
		if ((reinterpret_cast<uintptr_t>(errors) & 7u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose error records must be 8 byte aligned");
		if ((reinterpret_cast<uintptr_t>(desc->worst) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the worst pose error record must be 16 byte aligned");
		if (desc->reserved[0] != 0 || desc->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a pose error desc are 0");
		out_rows = { std::min(raw_pose_stride_bytes, lossy_pose_stride_bytes) / 48, true, "two of them are too large for the pose error measure" };
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_rows_launch_shape_of(context, out_rows, false, 0, shape); shape_status != ACLHIP_OK)
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

	// ---- 3x4 matrices of a pose buffer (aclhip_pose_matrices_batch; pose_matrices_kernel) -------------------------------------------------

	// What aclhip_pose_matrices_batch checks of its arguments before any device call; every refusal leaves a message, with or without a
	// context. The rows that shape the launch: both -- an image holds min(local_pose_stride_bytes / 48, matrix_stride_bytes / 64)
	// transforms (a matrix takes the three quads of its QVV record).
	aclhip_status check_pose_matrices(aclhip_context* context, const void* local_poses, uint64_t local_pose_stride_bytes, uint32_t num_instances,
		const aclhip_pose_matrices_desc* desc, const void* matrices, uint64_t matrix_stride_bytes, pose_rows& out_rows)
	{
		if (desc == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose matrices desc");
		if (local_poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null local pose buffer");
		if (matrices == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null matrix buffer");
		if (const aclhip_status status = check_names_skeleton(context, "a pose matrices desc names", desc->skeleton, desc->instance_skeletons); status != ACLHIP_OK)
			return status;
		if (desc->layout != ACLHIP_MATRIX_3X4F_64)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown matrix layout %u", desc->layout);
		if (const aclhip_status status = check_rows_aligned(context, { { "local pose", local_poses, local_pose_stride_bytes }, { "matrix", matrices, matrix_stride_bytes } }); status != ACLHIP_OK)
			return status;
		if (desc->reserved[0] != 0 || desc->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a pose matrices desc are 0");
		out_rows = { std::min(local_pose_stride_bytes / 48, matrix_stride_bytes / 64), false, "too large for the pose matrices" };
		consumer_launch_shape shape;
		if (const aclhip_status shape_status = pose_rows_launch_shape_of(context, out_rows, false, 0, shape); shape_status != ACLHIP_OK)
			return shape_status;
		// records differ in size: there is no in place form, and no other overlap either (the skeleton list is only read as well)
		if (pose_ranges_overlap(matrices, matrix_stride_bytes, local_poses, local_pose_stride_bytes, num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the matrix rows overlap the local pose rows: a matrix is larger than its transform, there is no in place form");
		if (desc->instance_skeletons != nullptr && pose_ranges_overlap(matrices, matrix_stride_bytes, desc->instance_skeletons, sizeof(aclhip_skeleton), num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the matrix rows overlap the skeleton list");
		return ACLHIP_OK;
	}
}

// include/aclhip.h states the definition. The argument checks need no device, come first and leave a message, with or without a context.
extern "C" aclhip_status aclhip_transform_poses_batch(aclhip_context* context, const void* local_poses, uint64_t local_pose_stride_bytes, uint32_t num_instances,
	const aclhip_pose_buffer_consumers* consumers, void* poses, uint64_t pose_stride_bytes, void* stream_handle)
{
	pose_rows rows;
	const aclhip_status status = check_pose_buffer_consumers(context, local_poses, local_pose_stride_bytes, num_instances, consumers, poses, pose_stride_bytes, rows);
	if (status != ACLHIP_OK)
		return status;
	const bool object_space = consumers->object_space != 0;
	return launch_pose_rows(context, num_instances, stream_handle, rows, object_space, false, false, [&](hipStream_t stream, const consumer_launch_shape& shape, uint32_t num_blocks) -> aclhip_status
	{
		const bool has_additive = consumers->additive_format != ACLHIP_ADDITIVE_NONE;
		pose_buffer_launch launch = {};
		launch.head = pose_rows_head_of(context, consumers->skeleton, consumers->instance_skeletons);
		launch.shape = pose_rows_shape_of(context, num_instances, shape);
		launch.local_poses = static_cast<const uint8_t*>(local_poses);
		launch.local_pose_stride_bytes = local_pose_stride_bytes;
		launch.additive_poses = has_additive ? static_cast<const uint8_t*>(consumers->additive_poses) : nullptr;
		launch.additive_pose_stride_bytes = has_additive ? consumers->additive_pose_stride_bytes : 0;
		launch.poses = static_cast<uint8_t*>(poses);
		launch.pose_stride_bytes = pose_stride_bytes;
		launch.additive_format = consumers->additive_format;

		// five instantiations: object / none, object / buffer, local / buffer, and the two object forms with bounds
		if (consumers->bounds != nullptr)
		{
			const consumer_bounds_launch bounds = { static_cast<uint8_t*>(consumers->bounds->bounds), consumers->bounds->bone_flags };
			return launch_consumer_kernel(context, has_additive ? transform_poses_kernel<true, k_consumer_base_buffer, consumer_bounds_launch>
				: transform_poses_kernel<true, k_consumer_base_none, consumer_bounds_launch>, shape, num_blocks, 1, stream, launch, bounds);
		}
		if (!object_space)
			return launch_consumer_kernel(context, transform_poses_kernel<false, k_consumer_base_buffer>, shape, num_blocks, 1, stream, launch);
		return launch_consumer_kernel(context, has_additive ? transform_poses_kernel<true, k_consumer_base_buffer> : transform_poses_kernel<true, k_consumer_base_none>,
			shape, num_blocks, 1, stream, launch);
	});
}

// include/aclhip.h states the definition. The argument checks need no device, come first and leave a message, with or without a context.
// (the mask table with no mask registered yet: a table of no records -- every handle but the null handle is refused in the kernel)
extern "C" aclhip_status aclhip_blend_poses_batch(aclhip_context* context, const aclhip_pose_buffer_blend* blend, uint32_t num_instances, void* poses, uint64_t pose_stride_bytes,
	void* stream_handle)
{
	pose_rows rows;
	const aclhip_status status = check_pose_buffer_blend(context, blend, num_instances, poses, pose_stride_bytes, rows);
	if (status != ACLHIP_OK)
		return status;
	const bool object_space = blend->object_space != 0;
	return launch_pose_rows(context, num_instances, stream_handle, rows, object_space, false, false, [&](hipStream_t stream, const consumer_launch_shape& shape, uint32_t num_blocks) -> aclhip_status
	{
		pose_blend_launch launch = {};
		launch.head = pose_rows_head_of(context, blend->skeleton, blend->instance_skeletons);
		launch.shape = pose_rows_shape_of(context, num_instances, shape);
		launch.masks = context->blend_masks.d_records;
		launch.num_masks = context->blend_masks.d_records != nullptr ? ACLHIP_MAX_BLEND_MASKS : 0u;
		launch.layered = blend->mode == ACLHIP_BLEND_LAYERED ? 1u : 0u;
		launch.instance_masks = blend->instance_masks;
		launch.weights = blend->weights;
		for (uint32_t k = 0; k < blend->num_buffers; ++k)
		{
			launch.buffers[k] = static_cast<const uint8_t*>(blend->buffers[k]);
			launch.buffer_stride_bytes[k] = blend->buffer_stride_bytes[k];
		}
		launch.poses = static_cast<uint8_t*>(poses);
		launch.pose_stride_bytes = pose_stride_bytes;

		switch (blend->num_buffers)
		{
		case 2: return launch_blend_poses_of<2>(context, shape, num_blocks, stream, launch, object_space, blend->bounds);
		case 3: return launch_blend_poses_of<3>(context, shape, num_blocks, stream, launch, object_space, blend->bounds);
		default: return launch_blend_poses_of<4>(context, shape, num_blocks, stream, launch, object_space, blend->bounds);
		}
	});
}

// include/aclhip.h states the definition. The argument checks need no device, come first and leave a message, with or without a context.
// (the kernel has no walk: its shape is without a walk schedule, whatever the context holds -- not in object space)
extern "C" aclhip_status aclhip_inverse_transform_poses_batch(aclhip_context* context, const void* source_poses, uint64_t source_pose_stride_bytes, uint32_t num_instances,
	const aclhip_pose_buffer_inverse* inverse, void* poses, uint64_t pose_stride_bytes, void* stream_handle)
{
	pose_rows rows;
	const aclhip_status status = check_pose_buffer_inverse(context, source_poses, source_pose_stride_bytes, num_instances, inverse, poses, pose_stride_bytes, rows);
	if (status != ACLHIP_OK)
		return status;
	return launch_pose_rows(context, num_instances, stream_handle, rows, false, false, false, [&](hipStream_t stream, const consumer_launch_shape& shape, uint32_t num_blocks) -> aclhip_status
	{
		const bool has_base = inverse->additive_format != ACLHIP_ADDITIVE_NONE;
		pose_inverse_launch launch = {};
		launch.head = pose_rows_head_of(context, inverse->skeleton, inverse->instance_skeletons);
		launch.shape = pose_rows_shape_of(context, num_instances, shape);
		launch.source_poses = static_cast<const uint8_t*>(source_poses);
		launch.source_pose_stride_bytes = source_pose_stride_bytes;
		launch.base_poses = has_base ? static_cast<const uint8_t*>(inverse->base_poses) : nullptr;
		launch.base_pose_stride_bytes = has_base ? inverse->base_pose_stride_bytes : 0;
		launch.poses = static_cast<uint8_t*>(poses);
		launch.pose_stride_bytes = pose_stride_bytes;
		launch.additive_format = inverse->additive_format;

		// three instantiations: local / none, local / base, no-local / base
		if (inverse->local_space == 0)
			return launch_consumer_kernel(context, inverse_transform_poses_kernel<false, true>, shape, num_blocks, 1, stream, launch);
		return launch_consumer_kernel(context, has_base ? inverse_transform_poses_kernel<true, true> : inverse_transform_poses_kernel<true, false>, shape, num_blocks, 1, stream, launch);
	});
}

// include/aclhip.h states the definition. The argument checks need no device, come first and leave a message, with or without a context.
// The worst record is a second, one workgroup launch over the instances' records on the same stream -- the only launch of a batch of none.
extern "C" aclhip_status aclhip_measure_pose_error_metric_batch(aclhip_context* context, const void* raw_poses, uint64_t raw_pose_stride_bytes, const void* lossy_poses,
	uint64_t lossy_pose_stride_bytes, uint32_t num_instances, const aclhip_pose_error_desc* desc, uint32_t metric, aclhip_pose_error* errors, void* stream_handle)
{
	pose_rows rows;
	const aclhip_status status = check_pose_error(context, raw_poses, raw_pose_stride_bytes, lossy_poses, lossy_pose_stride_bytes, num_instances, desc, errors, rows);
	if (status != ACLHIP_OK)
		return status;
	if (metric > ACLHIP_METRIC_QVVF_MATRIX3X4F)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown error metric %u", metric);
	if (metric == ACLHIP_METRIC_QVVF_MATRIX3X4F && desc->additive_format != ACLHIP_ADDITIVE_NONE)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the matrix error metric takes no additive format: apply_additive_to_base is defined over QVV poses only");
	const bool object_space = desc->object_space != 0;
	return launch_pose_rows(context, num_instances, stream_handle, rows, object_space, false, desc->worst != nullptr, [&](hipStream_t stream, const consumer_launch_shape& shape, uint32_t num_blocks) -> aclhip_status
	{
		if (num_instances != 0)
		{
			const bool has_base = desc->additive_format != ACLHIP_ADDITIVE_NONE;
			pose_error_launch launch = {};
			launch.head = pose_rows_head_of(context, desc->skeleton, desc->instance_skeletons);
			launch.shape = pose_rows_shape_of(context, num_instances, shape);
			launch.raw_poses = static_cast<const uint8_t*>(raw_poses);
			launch.raw_pose_stride_bytes = raw_pose_stride_bytes;
			launch.lossy_poses = static_cast<const uint8_t*>(lossy_poses);
			launch.lossy_pose_stride_bytes = lossy_pose_stride_bytes;
			launch.base_poses = has_base ? static_cast<const uint8_t*>(desc->base_poses) : nullptr;
			launch.base_pose_stride_bytes = has_base ? desc->base_pose_stride_bytes : 0;
			launch.shell_distances = desc->shell_distances;
			launch.num_shell_distances = desc->num_shell_distances;
			launch.shell_distance = desc->shell_distance;
			launch.bone_errors = reinterpret_cast<uint8_t*>(desc->bone_errors);
			launch.bone_error_stride_bytes = desc->bone_error_stride_bytes;
			launch.errors = reinterpret_cast<pose_error_record*>(errors);
			launch.additive_format = desc->additive_format;

			// four instantiations: object / local x base / none, and the matrix metric's two: object / local (it takes no base)
			const auto kernel = metric == ACLHIP_METRIC_QVVF_MATRIX3X4F
				? (object_space ? measure_pose_error_kernel<true, false, true> : measure_pose_error_kernel<false, false, true>)
				: object_space ? (has_base ? measure_pose_error_kernel<true, true, false> : measure_pose_error_kernel<true, false, false>)
				: (has_base ? measure_pose_error_kernel<false, true, false> : measure_pose_error_kernel<false, false, false>);
			// two waves per instance: one per image
			if (const aclhip_status launch_status = launch_consumer_kernel(context, kernel, shape, num_blocks, 2, stream, launch); launch_status != ACLHIP_OK)
				return launch_status;
		}
		if (desc->worst != nullptr)
		{
			hipLaunchKernelGGL(pose_error_worst_kernel, dim3(1), dim3(k_pose_error_worst_threads), 0, stream, reinterpret_cast<const pose_error_record*>(errors), num_instances,
				reinterpret_cast<u32x4*>(desc->worst));
			ACLHIP_CHECK_HIP(context, hipGetLastError());
		}
		return ACLHIP_OK;
	});
}

// ACLHIP_METRIC_QVVF of the call above: one host path
extern "C" aclhip_status aclhip_measure_pose_error_batch(aclhip_context* context, const void* raw_poses, uint64_t raw_pose_stride_bytes, const void* lossy_poses,
	uint64_t lossy_pose_stride_bytes, uint32_t num_instances, const aclhip_pose_error_desc* desc, aclhip_pose_error* errors, void* stream)
{
	return aclhip_measure_pose_error_metric_batch(context, raw_poses, raw_pose_stride_bytes, lossy_poses, lossy_pose_stride_bytes, num_instances, desc, ACLHIP_METRIC_QVVF, errors, stream);
}

// include/aclhip.h states the definition. The argument checks need no device, come first and leave a message, with or without a context.
extern "C" aclhip_status aclhip_pose_matrices_batch(aclhip_context* context, const void* local_poses, uint64_t local_pose_stride_bytes, uint32_t num_instances,
	const aclhip_pose_matrices_desc* desc, void* matrices, uint64_t matrix_stride_bytes, void* stream_handle)
{
	pose_rows rows;
	const aclhip_status status = check_pose_matrices(context, local_poses, local_pose_stride_bytes, num_instances, desc, matrices, matrix_stride_bytes, rows);
	if (status != ACLHIP_OK)
		return status;
	const bool object_space = desc->object_space != 0;
	return launch_pose_rows(context, num_instances, stream_handle, rows, object_space, false, false, [&](hipStream_t stream, const consumer_launch_shape& shape, uint32_t num_blocks) -> aclhip_status
	{
		pose_matrices_launch launch = {};
		launch.head = pose_rows_head_of(context, desc->skeleton, desc->instance_skeletons);
		launch.shape = pose_rows_shape_of(context, num_instances, shape);
		launch.local_poses = static_cast<const uint8_t*>(local_poses);
		launch.local_pose_stride_bytes = local_pose_stride_bytes;
		launch.matrices = static_cast<uint8_t*>(matrices);
		launch.matrix_stride_bytes = matrix_stride_bytes;
		return launch_consumer_kernel(context, object_space ? pose_matrices_kernel<true> : pose_matrices_kernel<false>, shape, num_blocks, 1, stream, launch);
	});
}
