// host_transform_compress.inl -- part of aclhip.hip (one translation unit; included there behind host_scalar_compress.inl, not compiled on its own).
// Host side of aclhip_compress_raw_tracks_batch (kernels_transform_compress.inl): the two sizes a caller needs, the argument checks and
// the four launches. include/aclhip.h states the definition.

static_assert(sizeof(aclhip_transform_compress_desc) == 80, "header layout");
static_assert(offsetof(aclhip_transform_compress_desc, default_pose) == 8 && offsetof(aclhip_transform_compress_desc, num_table_tracks) == 40
	&& offsetof(aclhip_transform_compress_desc, shell_distance) == 48 && offsetof(aclhip_transform_compress_desc, workspace) == 56
	&& offsetof(aclhip_transform_compress_desc, reserved) == 64, "header layout");

namespace
{
	constexpr uint32_t k_transform_compress_flags = ACLHIP_COMPRESS_OPTIMIZE_LOOPS | ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES | ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS;

	// the three parts of the workspace, each rounded up to 16 bytes (128 bits wide: see aclhip_scalar_compress_workspace_bytes)
	unsigned __int128 transform_workspace_part(unsigned __int128 bytes) { return (bytes + 15u) & ~(unsigned __int128)15; }
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
	const unsigned __int128 bytes = transform_workspace_part(n * sizeof(scalar_compress_instance)) + transform_workspace_part(n * max_tracks)
		+ transform_workspace_part(n * max_tracks * 3u * sizeof(uint16_t));
	return bytes > (UINT64_MAX & ~uint64_t(15)) ? UINT64_MAX & ~uint64_t(15) : uint64_t(bytes);
}

namespace
{
	// What the launch checks of its arguments before any device call; every refusal leaves a message, with or without a context
	aclhip_status check_transform_compress(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances, const aclhip_transform_compress_desc* desc,
		const void* blobs, uint64_t blob_stride_bytes, const aclhip_compress_result* results)
	{
		if (raws == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null raw track handles");
		if (desc == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null transform compress desc");
		if (blobs == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null blob buffer");
		if (results == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null compress results");
		if (desc->workspace == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null workspace");
		if (blob_stride_bytes == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a blob stride of 0");
		if ((reinterpret_cast<uintptr_t>(blobs) & 15u) != 0 || (blob_stride_bytes & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the blob buffer and its stride must be 16 byte aligned");
		if ((reinterpret_cast<uintptr_t>(desc->workspace) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the workspace must be 16 byte aligned");
		if ((reinterpret_cast<uintptr_t>(results) & 7u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "compress results must be 8 byte aligned");
		if ((reinterpret_cast<uintptr_t>(desc->default_pose) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the default pose must be 16 byte aligned");
		if (((reinterpret_cast<uintptr_t>(desc->parent_indices) | reinterpret_cast<uintptr_t>(desc->track_precisions) | reinterpret_cast<uintptr_t>(desc->track_shell_distances)) & 3u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the track tables must be 4 byte aligned");
		if ((desc->flags & ~k_transform_compress_flags) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown compress flags 0x%x", desc->flags);
		if (desc->reserved[0] != 0 || desc->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a transform compress desc are 0");
		if (!std::isfinite(desc->precision) || desc->precision < 0.0f)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a precision of %g: it must be finite and not negative", double(desc->precision));
		if (!std::isfinite(desc->shell_distance) || desc->shell_distance < 0.0f)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a shell distance of %g: it must be finite and not negative", double(desc->shell_distance));
		const bool has_table = desc->default_pose != nullptr || desc->parent_indices != nullptr || desc->track_precisions != nullptr || desc->track_shell_distances != nullptr;
		if (has_table && desc->num_table_tracks == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a track table with a count of 0");
		if (desc->max_tracks == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a transform compress desc of 0 max_tracks");

		// what is written overlaps nothing that is read and no other output (the inputs are only read and may share bytes)
		struct byte_range { const char* name; const void* pointer; unsigned __int128 bytes; };
		const unsigned __int128 n = num_instances, table = desc->num_table_tracks;
		const byte_range outputs[] = {
			{ "the blob rows", blobs, n * blob_stride_bytes },
			{ "the compress results", results, n * sizeof(aclhip_compress_result) },
			{ "the workspace", desc->workspace, aclhip_transform_compress_workspace_bytes(num_instances, desc->max_tracks) },
		};
		const byte_range inputs[] = {
			{ "the raw track handles", raws, n * sizeof(aclhip_raw_tracks) },
			{ "the default pose", desc->default_pose, desc->default_pose != nullptr ? table * 48u : 0 },
			{ "the parent indices", desc->parent_indices, desc->parent_indices != nullptr ? table * sizeof(uint32_t) : 0 },
			{ "the track precisions", desc->track_precisions, desc->track_precisions != nullptr ? table * sizeof(float) : 0 },
			{ "the track shell distances", desc->track_shell_distances, desc->track_shell_distances != nullptr ? table * sizeof(float) : 0 },
		};
		for (size_t o = 0; o < std::size(outputs); ++o)
		{
			for (const byte_range& input : inputs)
				if (byte_ranges_overlap(outputs[o].pointer, outputs[o].bytes, input.pointer, input.bytes))
					return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s overlap %s", outputs[o].name, input.name);
			for (size_t other = o + 1; other < std::size(outputs); ++other)
				if (byte_ranges_overlap(outputs[o].pointer, outputs[o].bytes, outputs[other].pointer, outputs[other].bytes))
					return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s overlap %s", outputs[o].name, outputs[other].name);
		}
		return ACLHIP_OK;
	}
}

// The four launches, in stream order on `stream`: each reads what the one before it left in the workspace. Shapes come from the arguments
// alone -- the handles live on the device --: the analysis takes max_tracks waves per instance (an array holds at most 0xFFFF tracks), the
// stream a wave per k_compress_dwords_per_lane * 64 dwords of a row. Nothing is uploaded; the table is read under the registry lock.
extern "C" aclhip_status aclhip_compress_raw_tracks_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_transform_compress_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
{
	const aclhip_status status = check_transform_compress(context, raws, num_instances, desc, blobs, blob_stride_bytes, results);
	if (status != ACLHIP_OK)
		return status;
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	if (num_instances == 0)
		return ACLHIP_OK;

	device_guard guard(context->device);
	hipStream_t stream = static_cast<hipStream_t>(stream_handle);
	std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
	if (context->raw_tracks.d_records == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no raw track array was ever registered with this context");
	note_launch_stream(context, stream);

	const bool has_table = desc->default_pose != nullptr || desc->parent_indices != nullptr || desc->track_precisions != nullptr || desc->track_shell_distances != nullptr;
	transform_compress_launch launch = {};
	launch.arrays = context->raw_tracks.d_records;
	launch.num_arrays = ACLHIP_MAX_RAW_TRACKS;
	launch.num_instances = num_instances;
	launch.raws = raws;
	launch.default_pose = static_cast<const f32x4*>(desc->default_pose);
	launch.parent_indices = desc->parent_indices;
	launch.track_precisions = desc->track_precisions;
	launch.track_shell_distances = desc->track_shell_distances;
	launch.table_tracks = has_table ? desc->num_table_tracks : 0xFFFFFFFFu;
	launch.flags = desc->flags;
	launch.precision = desc->precision;
	launch.shell_distance = desc->shell_distance;
	launch.max_tracks = desc->max_tracks;
	uint8_t* workspace = static_cast<uint8_t*>(desc->workspace);
	launch.instances = reinterpret_cast<scalar_compress_instance*>(workspace);
	launch.track_flags = workspace + uint64_t(transform_workspace_part((unsigned __int128)num_instances * sizeof(scalar_compress_instance)));
	launch.animated = reinterpret_cast<uint16_t*>(launch.track_flags + uint64_t(transform_workspace_part((unsigned __int128)num_instances * desc->max_tracks)));
	launch.blobs = static_cast<uint8_t*>(blobs);
	launch.blob_stride_bytes = blob_stride_bytes;
	launch.results = reinterpret_cast<uint2*>(results);
	launch.rejected_count = context->d_rejected;

	// (the wave index of the stream kernel is 32 bits wide: a batch too large for its share of waves loops)
	constexpr uint64_t dwords_per_wave = uint64_t(k_wave_size) * k_compress_dwords_per_lane;
	uint64_t waves_per_instance = std::max<uint64_t>((std::min<uint64_t>(blob_stride_bytes, uint64_t(1) << 32) / 4 + dwords_per_wave - 1) / dwords_per_wave, 1);
	waves_per_instance = std::min<uint64_t>(waves_per_instance, std::max<uint64_t>(0xFFFFFFF0ull / num_instances, 1));
	launch.waves_per_instance = uint32_t(waves_per_instance);

	// the hash kernel is the scalar compressor's: it reads the instance records and the rows
	scalar_compress_launch hash_launch = {};
	hash_launch.num_instances = num_instances;
	hash_launch.instances = launch.instances;
	hash_launch.blobs = launch.blobs;
	hash_launch.blob_stride_bytes = blob_stride_bytes;

	constexpr uint32_t block_size = k_compress_waves_per_block * k_wave_size;
	const uint32_t instance_blocks = (num_instances - 1) / k_compress_waves_per_block + 1;
	const uint32_t track_blocks = (std::min<uint32_t>(desc->max_tracks, 0xFFFFu) - 1) / k_compress_waves_per_block + 1;
	const uint32_t stream_blocks = uint32_t((uint64_t(num_instances) * waves_per_instance - 1) / k_compress_waves_per_block + 1);

	// measurement knob (the lab library alone reads it, per call): only the first k launches -- what each phase costs (tools/transform_compress.py)
	const char* phases_knob = lab_knob("ACLHIP_TRANSFORM_COMPRESS_PHASES");
	const int phases = phases_knob != nullptr ? std::atoi(phases_knob) : 4;

	hipLaunchKernelGGL(transform_compress_analyze_kernel, dim3(track_blocks, std::min<uint32_t>(num_instances, 65535u)), dim3(block_size), 0, stream, launch);
	ACLHIP_CHECK_HIP(context, hipGetLastError());
	if (phases >= 2)
	{
		hipLaunchKernelGGL(transform_compress_layout_kernel, dim3(instance_blocks), dim3(block_size), 0, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
	}
	if (phases >= 3)
	{
		hipLaunchKernelGGL(transform_compress_stream_kernel, dim3(stream_blocks), dim3(block_size), 0, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
	}
	if (phases >= 4)
	{
		hipLaunchKernelGGL(scalar_compress_hash_kernel, dim3(num_instances), dim3(k_wave_size), 0, stream, hash_launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
	}
	return ACLHIP_OK;
}
