// host_transform_compress.inl -- part of aclhip.hip (one translation unit; included there behind host_scalar_compress.inl, not compiled on its own).
// Host side of aclhip_compress_raw_tracks_batch (kernels_transform_compress.inl): the two sizes a caller needs, the argument checks and
// the four launches. What it shares with the scalar compressor -- the common checks, the launches' shapes and their front -- is in
// host_scalar_compress.inl. include/aclhip.h states the definition.

static_assert(sizeof(aclhip_transform_compress_desc) == 80, "header layout");
static_assert(offsetof(aclhip_transform_compress_desc, default_pose) == 8 && offsetof(aclhip_transform_compress_desc, num_table_tracks) == 40
	&& offsetof(aclhip_transform_compress_desc, shell_distance) == 48 && offsetof(aclhip_transform_compress_desc, workspace) == 56
	&& offsetof(aclhip_transform_compress_desc, reserved) == 64, "header layout");

namespace
{
	constexpr uint32_t k_transform_compress_flags = ACLHIP_COMPRESS_OPTIMIZE_LOOPS | ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES | ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS;

	// the three parts of the workspace, each rounded up to 16 bytes (128 bits wide: see aclhip_scalar_compress_workspace_bytes)
	unsigned __int128 transform_workspace_part(unsigned __int128 bytes) { return (bytes + 15u) & ~(unsigned __int128)15; }

	// one count (num_table_tracks) for every per-track table a desc names
	bool transform_compress_has_table(const aclhip_transform_compress_desc& desc)
	{
		return desc.default_pose != nullptr || desc.parent_indices != nullptr || desc.track_precisions != nullptr || desc.track_shell_distances != nullptr;
	}
}

extern "C" uint64_t aclhip_transform_compress_bound(uint32_t num_tracks, uint32_t num_samples, uint32_t flags)
{
	// headers, 2 bits per sub-track in words of 16, every sub-track animated (a constant one takes its 16 or 12 bytes once, and an array
	// has a sample), metadata or the tail
	const unsigned __int128 tracks = num_tracks;
	unsigned __int128 bytes = k_transform_blob_headers + 12u * ((tracks + 15u) / 16u) + 40u * tracks * num_samples;
	if ((flags & (ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES | ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS)) != 0)
		bytes += 4u * tracks + ((flags & ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS) != 0 ? 48u * tracks : 0u) + sizeof(optional_metadata_header);
	else
		bytes += 15u;
	return bytes > (UINT64_MAX & ~uint64_t(15)) ? UINT64_MAX & ~uint64_t(15) : (uint64_t(bytes) + 15u) & ~uint64_t(15);
}

extern "C" uint64_t aclhip_transform_compress_workspace_bytes(uint32_t num_instances, uint32_t max_tracks)
{
	const unsigned __int128 n = num_instances;
	const unsigned __int128 bytes = transform_workspace_part(n * sizeof(compress_instance)) + transform_workspace_part(n * max_tracks)
		+ transform_workspace_part(n * max_tracks * 3u * sizeof(uint16_t));
	return bytes > (UINT64_MAX & ~uint64_t(15)) ? UINT64_MAX & ~uint64_t(15) : uint64_t(bytes);
}

namespace
{
	// What the launch checks of its arguments before any device call, its own between the parts both compressors check (host_scalar_compress.inl)
	aclhip_status check_transform_compress(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances, const aclhip_transform_compress_desc* desc,
		const void* blobs, uint64_t blob_stride_bytes, const aclhip_compress_result* results)
	{
		if (const aclhip_status status = check_compress_buffers(context, "transform", "raw track", raws, desc, blobs, blob_stride_bytes, results); status != ACLHIP_OK)
			return status;
		if ((reinterpret_cast<uintptr_t>(desc->default_pose) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the default pose must be 16 byte aligned");
		if (((reinterpret_cast<uintptr_t>(desc->parent_indices) | reinterpret_cast<uintptr_t>(desc->track_precisions) | reinterpret_cast<uintptr_t>(desc->track_shell_distances)) & 3u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the track tables must be 4 byte aligned");
		if (const aclhip_status status = check_compress_settings(context, "transform", *desc, k_transform_compress_flags); status != ACLHIP_OK)
			return status;
		if (!std::isfinite(desc->shell_distance) || desc->shell_distance < 0.0f)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a shell distance of %g: it must be finite and not negative", double(desc->shell_distance));
		if (transform_compress_has_table(*desc) && desc->num_table_tracks == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a track table with a count of 0");
		const unsigned __int128 n = num_instances, table = desc->num_table_tracks;
		return check_compress_ranges(context, "transform", *desc, aclhip_transform_compress_workspace_bytes(num_instances, desc->max_tracks), num_instances, blobs, blob_stride_bytes, results,
			{
				{ "the raw track handles", raws, n * sizeof(aclhip_raw_tracks) },
				{ "the default pose", desc->default_pose, desc->default_pose != nullptr ? table * 48u : 0 },
				{ "the parent indices", desc->parent_indices, desc->parent_indices != nullptr ? table * sizeof(uint32_t) : 0 },
				{ "the track precisions", desc->track_precisions, desc->track_precisions != nullptr ? table * sizeof(float) : 0 },
				{ "the track shell distances", desc->track_shell_distances, desc->track_shell_distances != nullptr ? table * sizeof(float) : 0 },
			});
	}
}

// The four launches
extern "C" aclhip_status aclhip_compress_raw_tracks_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_transform_compress_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
{
	const aclhip_status status = check_transform_compress(context, raws, num_instances, desc, blobs, blob_stride_bytes, results);
	if (status != ACLHIP_OK)
		return status;
	return launch_compress(context, &aclhip_context::raw_tracks, num_instances, stream_handle, [&](hipStream_t stream) -> aclhip_status
	{
		const compress_launch_shape shape = compress_launch_shape_of(num_instances, desc->max_tracks, blob_stride_bytes, "ACLHIP_TRANSFORM_COMPRESS_PHASES");
		transform_compress_launch launch = {};
		launch.arrays = context->raw_tracks.d_records;
		launch.num_arrays = ACLHIP_MAX_RAW_TRACKS;
		launch.num_instances = num_instances;
		launch.raws = raws;
		launch.default_pose = static_cast<const f32x4*>(desc->default_pose);
		launch.parent_indices = desc->parent_indices;
		launch.track_precisions = desc->track_precisions;
		launch.track_shell_distances = desc->track_shell_distances;
		launch.table_tracks = transform_compress_has_table(*desc) ? desc->num_table_tracks : 0xFFFFFFFFu;
		launch.flags = desc->flags;
		launch.precision = desc->precision;
		launch.shell_distance = desc->shell_distance;
		launch.max_tracks = desc->max_tracks;
		uint8_t* workspace = static_cast<uint8_t*>(desc->workspace);
		launch.instances = reinterpret_cast<compress_instance*>(workspace);
		launch.track_flags = workspace + uint64_t(transform_workspace_part((unsigned __int128)num_instances * sizeof(compress_instance)));
		launch.animated = reinterpret_cast<uint16_t*>(launch.track_flags + uint64_t(transform_workspace_part((unsigned __int128)num_instances * desc->max_tracks)));
		launch.blobs = static_cast<uint8_t*>(blobs);
		launch.blob_stride_bytes = blob_stride_bytes;
		launch.results = reinterpret_cast<uint2*>(results);
		launch.waves_per_instance = shape.waves_per_instance;
		launch.rejected_count = context->d_rejected;
		const compress_hash_launch hash_launch = { launch.instances, num_instances, launch.blobs, blob_stride_bytes };

		hipLaunchKernelGGL(transform_compress_analyze_kernel, shape.track_blocks, dim3(shape.block_size), 0, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
		if (shape.phases >= 2)
		{
			hipLaunchKernelGGL(transform_compress_layout_kernel<false>, dim3(shape.instance_blocks), dim3(shape.block_size), 0, stream, launch);
			ACLHIP_CHECK_HIP(context, hipGetLastError());
		}
		if (shape.phases >= 3)
		{
			hipLaunchKernelGGL(transform_compress_stream_kernel<false>, dim3(shape.stream_blocks), dim3(shape.block_size), 0, stream, launch);
			ACLHIP_CHECK_HIP(context, hipGetLastError());
		}
		if (shape.phases >= 4)
		{
			hipLaunchKernelGGL(compress_hash_kernel, dim3(num_instances), dim3(k_wave_size), 0, stream, hash_launch);
			ACLHIP_CHECK_HIP(context, hipGetLastError());
		}
		return ACLHIP_OK;
	});
}
