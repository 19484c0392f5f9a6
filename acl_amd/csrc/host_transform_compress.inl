// host_transform_compress.inl -- part of aclhip.hip (one translation unit; included there behind host_scalar_compress.inl, not compiled on its own).
// Host side of the two transform compressors, aclhip_compress_raw_tracks_batch (kernels_transform_compress.inl) and
// aclhip_compress_tracks_batch (kernels_tracks_compress.inl): the sizes a caller needs, and one argument check, one workspace layout,
// one launch record and one list of launches for both -- the raw call is the other with the full formats, no shell and its own words.
// What they share with the scalar compressor -- the cap of a size, the common checks, the launches' shapes, their front and their list
// of phases -- is in host_scalar_compress.inl. include/aclhip.h states the definitions.

static_assert(sizeof(aclhip_transform_compress_desc) == 80, "header layout");
static_assert(offsetof(aclhip_transform_compress_desc, default_pose) == 8 && offsetof(aclhip_transform_compress_desc, num_table_tracks) == 40
	&& offsetof(aclhip_transform_compress_desc, shell_distance) == 48 && offsetof(aclhip_transform_compress_desc, workspace) == 56
	&& offsetof(aclhip_transform_compress_desc, reserved) == 64, "header layout");
static_assert(sizeof(aclhip_compress_tracks_desc) == 96, "header layout");
static_assert(offsetof(aclhip_compress_tracks_desc, flags) == 12 && offsetof(aclhip_compress_tracks_desc, num_table_tracks) == 20
	&& offsetof(aclhip_compress_tracks_desc, default_pose) == 24 && offsetof(aclhip_compress_tracks_desc, track_shell_distances) == 48
	&& offsetof(aclhip_compress_tracks_desc, precision) == 56 && offsetof(aclhip_compress_tracks_desc, shell_distance) == 60
	&& offsetof(aclhip_compress_tracks_desc, workspace) == 64 && offsetof(aclhip_compress_tracks_desc, shell_metadata) == 72
	&& offsetof(aclhip_compress_tracks_desc, reserved) == 80, "header layout");

namespace
{
	constexpr uint32_t k_transform_compress_flags = ACLHIP_COMPRESS_OPTIMIZE_LOOPS | ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES | ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS;

	// The workspace: where each part begins and where the last one ends, each part rounded up to 16 bytes (128 bits wide: see
	// aclhip_scalar_compress_workspace_bytes). The raw call has the first three parts, aclhip_compress_tracks_batch the shells
	// ({ local shell distance, precision } per instance and track) behind them. The size functions and the launch record both read it.
	struct transform_workspace_layout
	{
		unsigned __int128 instances = 0, track_flags, animated, shells, total;
		transform_workspace_layout(uint32_t num_instances, uint32_t max_tracks, bool with_shells)
		{
			const auto part = [](unsigned __int128 bytes) { return (bytes + 15u) & ~(unsigned __int128)15; };
			const unsigned __int128 n = num_instances;
			track_flags = instances + part(n * sizeof(compress_instance));
			animated = track_flags + part(n * max_tracks);
			shells = animated + part(n * max_tracks * 3u * sizeof(uint16_t));
			total = shells + (with_shells ? part(n * max_tracks * sizeof(float2)) : 0);
		}
	};
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
	return compress_size_of(bytes);
}

extern "C" uint64_t aclhip_transform_compress_workspace_bytes(uint32_t num_instances, uint32_t max_tracks)
{
	return compress_size_of(transform_workspace_layout(num_instances, max_tracks, false).total);
}

extern "C" uint64_t aclhip_compress_tracks_workspace_bytes(uint32_t num_instances, uint32_t max_tracks)
{
	return compress_size_of(transform_workspace_layout(num_instances, max_tracks, true).total);
}

namespace
{
	// What an entry point says of itself: the word of its messages, the knob of its phases and whether its workspace holds shells. The
	// rest of what tells the two apart is in the desc: the formats and the shell metadata, 0 for the raw call.
	struct transform_compress_kind { const char* name; const char* phases_knob; bool with_shells; };

	// The kernels between the shell and the hash, per rotation format: quatf_full (the raw call's), quatf_drop_w_full
	struct transform_compress_kernels { void (*analyze)(transform_compress_launch), (*layout)(transform_compress_launch), (*stream)(transform_compress_launch); };
	const transform_compress_kernels k_transform_compress_kernels[2] =
	{
		{ transform_compress_analyze_kernel, transform_compress_layout_kernel<false>, transform_compress_stream_kernel<false> },
		{ tracks_compress_analyze_kernel, transform_compress_layout_kernel<true>, transform_compress_stream_kernel<true> },
	};

	// one count (num_table_tracks) for every per-track table a desc names
	bool transform_compress_has_table(const aclhip_compress_tracks_desc& desc)
	{
		return desc.default_pose != nullptr || desc.parent_indices != nullptr || desc.track_precisions != nullptr || desc.track_shell_distances != nullptr;
	}

	// What the launch checks of its arguments before any device call, its own between the parts every compressor checks
	// (host_scalar_compress.inl). The raw call's desc has no shell metadata and the full formats: those clauses pass.
	aclhip_status check_transform_compress(aclhip_context* context, const transform_compress_kind& kind, const aclhip_raw_tracks* raws, uint32_t num_instances,
		const aclhip_compress_tracks_desc* desc, const void* blobs, uint64_t blob_stride_bytes, const aclhip_compress_result* results)
	{
		if (const aclhip_status status = check_compress_buffers(context, kind.name, "raw track", raws, desc, blobs, blob_stride_bytes, results); status != ACLHIP_OK)
			return status;
		if ((reinterpret_cast<uintptr_t>(desc->default_pose) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the default pose must be 16 byte aligned");
		if (((reinterpret_cast<uintptr_t>(desc->parent_indices) | reinterpret_cast<uintptr_t>(desc->track_precisions) | reinterpret_cast<uintptr_t>(desc->track_shell_distances)) & 3u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the track tables must be 4 byte aligned");
		if ((reinterpret_cast<uintptr_t>(desc->shell_metadata) & 7u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the shell metadata must be 8 byte aligned");
		if (const aclhip_status status = check_compress_settings(context, kind.name, *desc, k_transform_compress_flags); status != ACLHIP_OK)
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
		if (transform_compress_has_table(*desc) && desc->num_table_tracks == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a track table with a count of 0");
		const unsigned __int128 n = num_instances, table = desc->num_table_tracks;
		byte_range ranges[] =
		{
			{}, {}, {},
			{ "the raw track handles", raws, n * sizeof(aclhip_raw_tracks) },
			{ "the default pose", desc->default_pose, desc->default_pose != nullptr ? table * 48u : 0 },
			{ "the parent indices", desc->parent_indices, desc->parent_indices != nullptr ? table * sizeof(uint32_t) : 0 },
			{ "the track precisions", desc->track_precisions, desc->track_precisions != nullptr ? table * sizeof(float) : 0 },
			{ "the track shell distances", desc->track_shell_distances, desc->track_shell_distances != nullptr ? table * sizeof(float) : 0 },
		};
		const uint64_t workspace_bytes = compress_size_of(transform_workspace_layout(num_instances, desc->max_tracks, kind.with_shells).total);
		if (const aclhip_status status = check_compress_ranges(context, kind.name, *desc, workspace_bytes, num_instances, blobs, blob_stride_bytes, results, ranges); status != ACLHIP_OK)
			return status;
		// the fourth output, in a pass of its own behind that one: it overlaps no other and nothing that is read
		const byte_range shell_metadata = { "the shell metadata", desc->shell_metadata, desc->shell_metadata != nullptr ? n * desc->max_tracks * sizeof(float2) : 0 };
		return check_no_overlap(context, &shell_metadata, 1, ranges, 8);
	}

	// Both entry points behind their own words: the check, the launch record and the launches -- four for quatf_full (the raw call's), the
	// shell in front of them and its own analysis for quatf_drop_w_full.
	aclhip_status compress_transform_tracks(aclhip_context* context, const transform_compress_kind& kind, const aclhip_raw_tracks* raws, uint32_t num_instances,
		const aclhip_compress_tracks_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
	{
		const aclhip_status status = check_transform_compress(context, kind, raws, num_instances, desc, blobs, blob_stride_bytes, results);
		if (status != ACLHIP_OK)
			return status;
		return launch_compress(context, &aclhip_context::raw_tracks, num_instances, stream_handle, [&](hipStream_t stream) -> aclhip_status
		{
			const compress_launch_shape shape = compress_launch_shape_of(num_instances, desc->max_tracks, blob_stride_bytes, kind.phases_knob);
			const transform_workspace_layout layout(num_instances, desc->max_tracks, kind.with_shells);
			uint8_t* workspace = static_cast<uint8_t*>(desc->workspace);
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
			launch.instances = reinterpret_cast<compress_instance*>(workspace + uint64_t(layout.instances));
			launch.track_flags = workspace + uint64_t(layout.track_flags);
			launch.animated = reinterpret_cast<uint16_t*>(workspace + uint64_t(layout.animated));
			launch.shells = kind.with_shells ? reinterpret_cast<float2*>(workspace + uint64_t(layout.shells)) : nullptr;
			launch.shell_metadata = static_cast<float2*>(desc->shell_metadata);
			launch.blobs = static_cast<uint8_t*>(blobs);
			launch.blob_stride_bytes = blob_stride_bytes;
			launch.results = reinterpret_cast<uint2*>(results);
			launch.waves_per_instance = shape.waves_per_instance;
			launch.rejected_count = context->d_rejected;
			const compress_hash_launch hash_launch = { launch.instances, num_instances, launch.blobs, blob_stride_bytes };

			// (the phases knob counts the call's own launches: four for quatf_full, five for quatf_drop_w_full)
			const bool drop_w = desc->rotation_format == k_rotation_quatf_drop_w_full;
			const transform_compress_kernels& kernels = k_transform_compress_kernels[drop_w ? 1 : 0];
			const dim3 block(shape.block_size);
			const compress_phase phases[] =
			{
				{ tracks_compress_shell_kernel, dim3(shape.instance_blocks), block, launch },
				{ kernels.analyze, shape.track_blocks, block, launch },
				{ kernels.layout, dim3(shape.instance_blocks), block, launch },
				{ kernels.stream, dim3(shape.stream_blocks), block, launch },
				{ compress_hash_kernel, dim3(num_instances), dim3(k_wave_size), hash_launch },
			};
			return launch_compress_phases(context, stream, shape.phases, phases + (drop_w ? 0 : 1), drop_w ? 5 : 4);
		});
	}
}

extern "C" aclhip_status aclhip_compress_raw_tracks_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_transform_compress_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
{
	// its desc as the larger one: the full formats (0) and no shell metadata
	aclhip_compress_tracks_desc as_tracks = {};
	if (desc != nullptr)
	{
		as_tracks.flags = desc->flags;
		as_tracks.max_tracks = desc->max_tracks;
		as_tracks.num_table_tracks = desc->num_table_tracks;
		as_tracks.default_pose = desc->default_pose;
		as_tracks.parent_indices = desc->parent_indices;
		as_tracks.track_precisions = desc->track_precisions;
		as_tracks.track_shell_distances = desc->track_shell_distances;
		as_tracks.precision = desc->precision;
		as_tracks.shell_distance = desc->shell_distance;
		as_tracks.workspace = desc->workspace;
		as_tracks.reserved[0] = desc->reserved[0];
		as_tracks.reserved[1] = desc->reserved[1];
	}
	return compress_transform_tracks(context, { "transform", "ACLHIP_TRANSFORM_COMPRESS_PHASES", false }, raws, num_instances, desc != nullptr ? &as_tracks : nullptr, blobs,
		blob_stride_bytes, results, stream_handle);
}

extern "C" aclhip_status aclhip_compress_tracks_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_compress_tracks_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
{
	return compress_transform_tracks(context, { "tracks", "ACLHIP_TRACKS_COMPRESS_PHASES", true }, raws, num_instances, desc, blobs, blob_stride_bytes, results, stream_handle);
}
