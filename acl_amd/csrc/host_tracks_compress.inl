// host_tracks_compress.inl -- part of aclhip.hip (one translation unit; included there behind host_transform_compress.inl, not compiled on its own).
// Host side of aclhip_compress_tracks_batch (kernels_tracks_compress.inl): the workspace size, the argument checks and the launches --
// the raw call's four for quatf_full, five for quatf_drop_w_full. The bound is aclhip_transform_compress_bound; the common checks, the
// launches' shapes and their front are host_scalar_compress.inl's. include/aclhip.h states the definition.

static_assert(sizeof(aclhip_compress_tracks_desc) == 96, "header layout");
static_assert(offsetof(aclhip_compress_tracks_desc, flags) == 12 && offsetof(aclhip_compress_tracks_desc, num_table_tracks) == 20
	&& offsetof(aclhip_compress_tracks_desc, default_pose) == 24 && offsetof(aclhip_compress_tracks_desc, track_shell_distances) == 48
	&& offsetof(aclhip_compress_tracks_desc, precision) == 56 && offsetof(aclhip_compress_tracks_desc, shell_distance) == 60
	&& offsetof(aclhip_compress_tracks_desc, workspace) == 64 && offsetof(aclhip_compress_tracks_desc, shell_metadata) == 72
	&& offsetof(aclhip_compress_tracks_desc, reserved) == 80, "header layout");

extern "C" uint64_t aclhip_compress_tracks_workspace_bytes(uint32_t num_instances, uint32_t max_tracks)
{
	// the raw call's three parts and { local shell distance, precision } per instance and track
	const unsigned __int128 n = num_instances;
	const unsigned __int128 bytes = transform_workspace_part(n * sizeof(compress_instance)) + transform_workspace_part(n * max_tracks)
		+ transform_workspace_part(n * max_tracks * 3u * sizeof(uint16_t)) + transform_workspace_part(n * max_tracks * sizeof(float2));
	return bytes > (UINT64_MAX & ~uint64_t(15)) ? UINT64_MAX & ~uint64_t(15) : uint64_t(bytes);
}

namespace
{
	bool compress_tracks_has_table(const aclhip_compress_tracks_desc& desc)
	{
		return desc.default_pose != nullptr || desc.parent_indices != nullptr || desc.track_precisions != nullptr || desc.track_shell_distances != nullptr;
	}

	// What the launch checks of its arguments before any device call: the raw call's checks in the raw call's order, the formats behind the settings
	aclhip_status check_compress_tracks(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances, const aclhip_compress_tracks_desc* desc,
		const void* blobs, uint64_t blob_stride_bytes, const aclhip_compress_result* results)
	{
		if (const aclhip_status status = check_compress_buffers(context, "tracks", "raw track", raws, desc, blobs, blob_stride_bytes, results); status != ACLHIP_OK)
			return status;
		if ((reinterpret_cast<uintptr_t>(desc->default_pose) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the default pose must be 16 byte aligned");
		if (((reinterpret_cast<uintptr_t>(desc->parent_indices) | reinterpret_cast<uintptr_t>(desc->track_precisions) | reinterpret_cast<uintptr_t>(desc->track_shell_distances)) & 3u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the track tables must be 4 byte aligned");
		if ((reinterpret_cast<uintptr_t>(desc->shell_metadata) & 7u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the shell metadata must be 8 byte aligned");
		if (const aclhip_status status = check_compress_settings(context, "tracks", *desc, k_transform_compress_flags); status != ACLHIP_OK)
			return status;
		if (!std::isfinite(desc->shell_distance) || desc->shell_distance < 0.0f)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a shell distance of %g: it must be finite and not negative", double(desc->shell_distance));
		if (desc->rotation_format == k_rotation_quatf_drop_w_variable)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "rotation format quatf_drop_w_variable is not built");
		if (desc->rotation_format != k_rotation_quatf_full && desc->rotation_format != k_rotation_quatf_drop_w_full)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a rotation format of %u: 0 (quatf_full) or 2 (quatf_drop_w_full)", desc->rotation_format);
		if (desc->translation_format == 1 || desc->scale_format == 1)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "vector format vector3f_variable is not built");
		if (desc->translation_format != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a translation format of %u: 0 (vector3f_full)", desc->translation_format);
		if (desc->scale_format != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a scale format of %u: 0 (vector3f_full)", desc->scale_format);
		if (compress_tracks_has_table(*desc) && desc->num_table_tracks == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a track table with a count of 0");
		const unsigned __int128 n = num_instances, table = desc->num_table_tracks;
		if (const aclhip_status status = check_compress_ranges(context, "tracks", *desc, aclhip_compress_tracks_workspace_bytes(num_instances, desc->max_tracks), num_instances, blobs,
				blob_stride_bytes, results,
				{
					{ "the raw track handles", raws, n * sizeof(aclhip_raw_tracks) },
					{ "the default pose", desc->default_pose, desc->default_pose != nullptr ? table * 48u : 0 },
					{ "the parent indices", desc->parent_indices, desc->parent_indices != nullptr ? table * sizeof(uint32_t) : 0 },
					{ "the track precisions", desc->track_precisions, desc->track_precisions != nullptr ? table * sizeof(float) : 0 },
					{ "the track shell distances", desc->track_shell_distances, desc->track_shell_distances != nullptr ? table * sizeof(float) : 0 },
				}); status != ACLHIP_OK)
			return status;
		// the fourth output: it overlaps no other and nothing that is read
		const unsigned __int128 metadata_bytes = desc->shell_metadata != nullptr ? n * desc->max_tracks * sizeof(float2) : 0;
		return check_no_overlap(context,
			{ { "the shell metadata", desc->shell_metadata, metadata_bytes } },
			{
				{ "the blob rows", blobs, n * blob_stride_bytes }, { "the compress results", results, n * sizeof(aclhip_compress_result) },
				{ "the workspace", desc->workspace, aclhip_compress_tracks_workspace_bytes(num_instances, desc->max_tracks) },
				{ "the raw track handles", raws, n * sizeof(aclhip_raw_tracks) },
				{ "the default pose", desc->default_pose, desc->default_pose != nullptr ? table * 48u : 0 },
				{ "the parent indices", desc->parent_indices, desc->parent_indices != nullptr ? table * sizeof(uint32_t) : 0 },
				{ "the track precisions", desc->track_precisions, desc->track_precisions != nullptr ? table * sizeof(float) : 0 },
				{ "the track shell distances", desc->track_shell_distances, desc->track_shell_distances != nullptr ? table * sizeof(float) : 0 },
			});
	}
}

extern "C" aclhip_status aclhip_compress_tracks_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_compress_tracks_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
{
	const aclhip_status status = check_compress_tracks(context, raws, num_instances, desc, blobs, blob_stride_bytes, results);
	if (status != ACLHIP_OK)
		return status;
	return launch_compress(context, &aclhip_context::raw_tracks, num_instances, stream_handle, [&](hipStream_t stream) -> aclhip_status
	{
		const compress_launch_shape shape = compress_launch_shape_of(num_instances, desc->max_tracks, blob_stride_bytes, "ACLHIP_TRACKS_COMPRESS_PHASES");
		transform_compress_launch launch = {};
		launch.arrays = context->raw_tracks.d_records;
		launch.num_arrays = ACLHIP_MAX_RAW_TRACKS;
		launch.num_instances = num_instances;
		launch.raws = raws;
		launch.default_pose = static_cast<const f32x4*>(desc->default_pose);
		launch.parent_indices = desc->parent_indices;
		launch.track_precisions = desc->track_precisions;
		launch.track_shell_distances = desc->track_shell_distances;
		launch.table_tracks = compress_tracks_has_table(*desc) ? desc->num_table_tracks : 0xFFFFFFFFu;
		launch.flags = desc->flags;
		launch.precision = desc->precision;
		launch.shell_distance = desc->shell_distance;
		launch.max_tracks = desc->max_tracks;
		uint8_t* workspace = static_cast<uint8_t*>(desc->workspace);
		launch.instances = reinterpret_cast<compress_instance*>(workspace);
		launch.track_flags = workspace + uint64_t(transform_workspace_part((unsigned __int128)num_instances * sizeof(compress_instance)));
		launch.animated = reinterpret_cast<uint16_t*>(launch.track_flags + uint64_t(transform_workspace_part((unsigned __int128)num_instances * desc->max_tracks)));
		launch.shells = reinterpret_cast<float2*>(reinterpret_cast<uint8_t*>(launch.animated)
			+ uint64_t(transform_workspace_part((unsigned __int128)num_instances * desc->max_tracks * 3u * sizeof(uint16_t))));
		launch.shell_metadata = static_cast<float2*>(desc->shell_metadata);
		launch.blobs = static_cast<uint8_t*>(blobs);
		launch.blob_stride_bytes = blob_stride_bytes;
		launch.results = reinterpret_cast<uint2*>(results);
		launch.waves_per_instance = shape.waves_per_instance;
		launch.rejected_count = context->d_rejected;
		const compress_hash_launch hash_launch = { launch.instances, num_instances, launch.blobs, blob_stride_bytes };
		const bool drop_w = desc->rotation_format == k_rotation_quatf_drop_w_full;
		int phase = 0;		// (the phases knob counts this call's launches: four for quatf_full, five for quatf_drop_w_full)

		if (drop_w)
		{
			hipLaunchKernelGGL(tracks_compress_shell_kernel, dim3(shape.instance_blocks), dim3(shape.block_size), 0, stream, launch);
			ACLHIP_CHECK_HIP(context, hipGetLastError());
			++phase;
		}
		if (shape.phases > phase++)
		{
			if (drop_w)
				hipLaunchKernelGGL(tracks_compress_analyze_kernel, shape.track_blocks, dim3(shape.block_size), 0, stream, launch);
			else
				hipLaunchKernelGGL(transform_compress_analyze_kernel, shape.track_blocks, dim3(shape.block_size), 0, stream, launch);
			ACLHIP_CHECK_HIP(context, hipGetLastError());
		}
		if (shape.phases > phase++)
		{
			if (drop_w)
				hipLaunchKernelGGL(transform_compress_layout_kernel<true>, dim3(shape.instance_blocks), dim3(shape.block_size), 0, stream, launch);
			else
				hipLaunchKernelGGL(transform_compress_layout_kernel<false>, dim3(shape.instance_blocks), dim3(shape.block_size), 0, stream, launch);
			ACLHIP_CHECK_HIP(context, hipGetLastError());
		}
		if (shape.phases > phase++)
		{
			if (drop_w)
				hipLaunchKernelGGL(transform_compress_stream_kernel<true>, dim3(shape.stream_blocks), dim3(shape.block_size), 0, stream, launch);
			else
				hipLaunchKernelGGL(transform_compress_stream_kernel<false>, dim3(shape.stream_blocks), dim3(shape.block_size), 0, stream, launch);
			ACLHIP_CHECK_HIP(context, hipGetLastError());
		}
		if (shape.phases > phase++)
		{
			hipLaunchKernelGGL(compress_hash_kernel, dim3(num_instances), dim3(k_wave_size), 0, stream, hash_launch);
			ACLHIP_CHECK_HIP(context, hipGetLastError());
		}
		return ACLHIP_OK;
	});
}
