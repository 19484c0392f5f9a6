// host_scalar_compress.inl -- part of aclhip.hip (one translation unit; included there behind host_raw_scalar_tracks.inl, not compiled on its own).
// Host side of aclhip_compress_raw_scalar_tracks_batch (kernels_scalar_compress.inl): the two sizes a caller needs, the argument checks
// and the five launches. include/aclhip.h states the definition.

static_assert(sizeof(aclhip_scalar_compress_desc) == 48, "header layout");
static_assert(sizeof(aclhip_compress_result) == 8, "header layout");

extern "C" uint64_t aclhip_scalar_compress_bound(uint32_t track_type, uint32_t num_tracks, uint32_t num_samples)
{
	const uint64_t num_components = raw_scalar_components_of(track_type);
	if (num_components == 0)
		return 0;
	// headers, one byte per track padded to 4, the larger of constants (C floats) and ranges (2 C floats), every track raw, the tail
	const uint64_t bytes = 52u + ((uint64_t(num_tracks) + 3u) & ~uint64_t(3)) + 8u * num_components * num_tracks + 4u * num_components * num_tracks * num_samples + 15u;
	return (bytes + 15u) & ~uint64_t(15);
}

extern "C" uint64_t aclhip_scalar_compress_workspace_bytes(uint32_t num_instances, uint32_t max_tracks)
{
	// (128 bits wide: 2^32 instances of 2^32 tracks do not wrap into a small number; what no address space holds is reported as the largest multiple of 16)
	const unsigned __int128 per_track = sizeof(scalar_compress_track) + sizeof(scalar_compress_animated);
	const unsigned __int128 bytes = (unsigned __int128)num_instances * sizeof(scalar_compress_instance) + (unsigned __int128)num_instances * max_tracks * per_track;
	return bytes > (UINT64_MAX & ~uint64_t(15)) ? UINT64_MAX & ~uint64_t(15) : (uint64_t(bytes) + 15u) & ~uint64_t(15);
}

namespace
{
	// What the launch checks of its arguments before any device call; every refusal leaves a message, with or without a context
	aclhip_status check_scalar_compress(aclhip_context* context, const aclhip_raw_scalar_tracks* raws, uint32_t num_instances, const aclhip_scalar_compress_desc* desc,
		const void* blobs, uint64_t blob_stride_bytes, const aclhip_compress_result* results)
	{
		if (raws == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null raw scalar track handles");
		if (desc == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null scalar compress desc");
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
		if ((desc->flags & ~ACLHIP_COMPRESS_OPTIMIZE_LOOPS) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown compress flags 0x%x", desc->flags);
		if (desc->reserved[0] != 0 || desc->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a scalar compress desc are 0");
		if (!std::isfinite(desc->precision) || desc->precision < 0.0f)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a precision of %g: it must be finite and not negative", double(desc->precision));
		if (desc->track_precisions != nullptr && desc->num_track_precisions == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "track_precisions with a count of 0");
		if (desc->max_tracks == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a scalar compress desc of 0 max_tracks");

		// what is written overlaps nothing that is read and no other output (the inputs are only read and may share bytes)
		struct byte_range { const char* name; const void* pointer; unsigned __int128 bytes; };
		const unsigned __int128 n = num_instances;
		const byte_range outputs[] = {
			{ "the blob rows", blobs, n * blob_stride_bytes },
			{ "the compress results", results, n * sizeof(aclhip_compress_result) },
			{ "the workspace", desc->workspace, aclhip_scalar_compress_workspace_bytes(num_instances, desc->max_tracks) },
		};
		const byte_range inputs[] = {
			{ "the raw scalar track handles", raws, n * sizeof(aclhip_raw_scalar_tracks) },
			{ "the track precisions", desc->track_precisions, desc->track_precisions != nullptr ? (unsigned __int128)desc->num_track_precisions * sizeof(float) : 0 },
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

// The five launches, in stream order on `stream`: each reads what the one before it left in the workspace. Shapes come from the arguments
// alone -- the handles live on the device --: the analysis takes max_tracks waves per instance (an array holds at most 0xFFFF tracks), the
// bit stream a wave per k_compress_dwords_per_lane * 64 dwords of a row. Nothing is uploaded; the table is read under the registry lock.
extern "C" aclhip_status aclhip_compress_raw_scalar_tracks_batch(aclhip_context* context, const aclhip_raw_scalar_tracks* raws, uint32_t num_instances,
	const aclhip_scalar_compress_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
{
	const aclhip_status status = check_scalar_compress(context, raws, num_instances, desc, blobs, blob_stride_bytes, results);
	if (status != ACLHIP_OK)
		return status;
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	if (num_instances == 0)
		return ACLHIP_OK;

	device_guard guard(context->device);
	hipStream_t stream = static_cast<hipStream_t>(stream_handle);
	std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
	if (context->raw_scalar_tracks.d_records == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no raw scalar track array was ever registered with this context");
	note_launch_stream(context, stream);

	scalar_compress_launch launch = {};
	launch.arrays = context->raw_scalar_tracks.d_records;
	launch.num_arrays = ACLHIP_MAX_RAW_SCALAR_TRACKS;
	launch.num_instances = num_instances;
	launch.raws = raws;
	launch.track_precisions = desc->track_precisions;
	launch.num_track_precisions = desc->track_precisions != nullptr ? desc->num_track_precisions : 0u;
	launch.precision = desc->precision;
	launch.optimize_loops = (desc->flags & ACLHIP_COMPRESS_OPTIMIZE_LOOPS) != 0 ? 1u : 0u;
	launch.max_tracks = desc->max_tracks;
	uint8_t* workspace = static_cast<uint8_t*>(desc->workspace);
	launch.instances = reinterpret_cast<scalar_compress_instance*>(workspace);
	launch.tracks = reinterpret_cast<scalar_compress_track*>(workspace + uint64_t(num_instances) * sizeof(scalar_compress_instance));
	launch.animated = reinterpret_cast<scalar_compress_animated*>(reinterpret_cast<uint8_t*>(launch.tracks) + uint64_t(num_instances) * desc->max_tracks * sizeof(scalar_compress_track));
	launch.blobs = static_cast<uint8_t*>(blobs);
	launch.blob_stride_bytes = blob_stride_bytes;
	launch.results = reinterpret_cast<uint2*>(results);
	launch.rejected_count = context->d_rejected;

	// (the wave index of the write kernel is 32 bits wide: a batch too large for its share of waves loops)
	constexpr uint64_t dwords_per_wave = uint64_t(k_wave_size) * k_compress_dwords_per_lane;
	uint64_t waves_per_instance = std::max<uint64_t>((std::min<uint64_t>(blob_stride_bytes, uint64_t(1) << 32) / 4 + dwords_per_wave - 1) / dwords_per_wave, 1);
	waves_per_instance = std::min<uint64_t>(waves_per_instance, std::max<uint64_t>(0xFFFFFFF0ull / num_instances, 1));
	launch.waves_per_instance = uint32_t(waves_per_instance);

	constexpr uint32_t block_size = k_compress_waves_per_block * k_wave_size;
	const uint32_t instance_blocks = (num_instances - 1) / k_compress_waves_per_block + 1;
	const uint32_t track_blocks = (std::min<uint32_t>(desc->max_tracks, 0xFFFFu) - 1) / k_compress_waves_per_block + 1;
	const uint32_t write_blocks = uint32_t((uint64_t(num_instances) * waves_per_instance - 1) / k_compress_waves_per_block + 1);

	// measurement knob (the lab library alone reads it, per call): only the first k launches -- what each phase costs (tools/scalar_compress.py)
	const char* phases_knob = lab_knob("ACLHIP_SCALAR_COMPRESS_PHASES");
	const int phases = phases_knob != nullptr ? std::atoi(phases_knob) : 5;

	hipLaunchKernelGGL(scalar_compress_prepare_kernel, dim3(instance_blocks), dim3(block_size), 0, stream, launch);
	ACLHIP_CHECK_HIP(context, hipGetLastError());
	if (phases >= 2)
	{
		hipLaunchKernelGGL(scalar_compress_analyze_kernel, dim3(track_blocks, std::min<uint32_t>(num_instances, 65535u)), dim3(block_size), 0, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
	}
	if (phases >= 3)
	{
		hipLaunchKernelGGL(scalar_compress_layout_kernel, dim3(instance_blocks), dim3(block_size), 0, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
	}
	if (phases >= 4)
	{
		hipLaunchKernelGGL(scalar_compress_write_kernel, dim3(write_blocks), dim3(block_size), 0, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
	}
	if (phases >= 5)
	{
		hipLaunchKernelGGL(scalar_compress_hash_kernel, dim3(num_instances), dim3(k_wave_size), 0, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
	}
	return ACLHIP_OK;
}
