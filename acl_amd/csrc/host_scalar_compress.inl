// host_scalar_compress.inl -- part of aclhip.hip (one translation unit; included there behind host_raw_scalar_tracks.inl, not compiled on its own).
// Host side of aclhip_compress_raw_scalar_tracks_batch (kernels_scalar_compress.inl): the two sizes a caller needs, the argument checks
// and the five launches -- and what the two transform compressors (host_transform_compress.inl) do the same way, stated once for all
// three: the cap of a size, the common checks, the launches' shapes, their front and their list of phases. include/aclhip.h states the
// definitions.

static_assert(sizeof(aclhip_scalar_compress_desc) == 48, "header layout");
static_assert(sizeof(aclhip_compress_result) == 8, "header layout");

namespace
{
	// A size computed 128 bits wide, rounded up to 16; what no address space holds is reported as the largest multiple of 16
	uint64_t compress_size_of(unsigned __int128 bytes)
	{
		constexpr uint64_t largest = UINT64_MAX & ~uint64_t(15);
		return bytes > largest ? largest : (uint64_t(bytes) + 15u) & ~uint64_t(15);
	}
}

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
	// (128 bits wide: 2^32 instances of 2^32 tracks do not wrap into a small number)
	const unsigned __int128 per_track = sizeof(scalar_compress_track) + sizeof(scalar_compress_animated);
	return compress_size_of((unsigned __int128)num_instances * sizeof(compress_instance) + (unsigned __int128)num_instances * max_tracks * per_track);
}

namespace
{
	// ---- what the compressors do alike (host_transform_compress.inl holds the other two) ---------------------------------------------------

	// What a compress launch checks of its arguments before any device call; every refusal leaves a message, with or without a context.
	// In three parts, and a kind's own checks stand where they stood between them: the pointers and their alignment (`kind` is the
	// word a desc goes by in the messages: "scalar compress"; a call that writes no blob rows has none to be null or misaligned),
	template<class desc_type>
	aclhip_status check_compress_buffers(aclhip_context* context, const char* kind, const char* handles, const void* raws, const desc_type* desc, const void* blobs,
		uint64_t blob_stride_bytes, const aclhip_compress_result* results, bool with_rows = true)
	{
		if (raws == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null %s handles", handles);
		if (desc == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null %s desc", kind);
		if (with_rows && blobs == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null blob buffer");
		if (results == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null compress results");
		if (desc->workspace == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null workspace");
		if (with_rows && blob_stride_bytes == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a blob stride of 0");
		if (with_rows && ((reinterpret_cast<uintptr_t>(blobs) & 15u) != 0 || (blob_stride_bytes & 15u) != 0))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the blob buffer and its stride must be 16 byte aligned");
		if ((reinterpret_cast<uintptr_t>(desc->workspace) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the workspace must be 16 byte aligned");
		if ((reinterpret_cast<uintptr_t>(results) & 7u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "compress results must be 8 byte aligned");
		return ACLHIP_OK;
	}

	// the settings,
	template<class desc_type>
	aclhip_status check_compress_settings(aclhip_context* context, const char* kind, const desc_type& desc, uint32_t known_flags)
	{
		if ((desc.flags & ~known_flags) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown compress flags 0x%x", desc.flags);
		if (desc.reserved[0] != 0 || desc.reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a %s desc are 0", kind);
		if (!std::isfinite(desc.precision) || desc.precision < 0.0f)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a precision of %g: it must be finite and not negative", double(desc.precision));
		return ACLHIP_OK;
	}

	// and max_tracks with the ranges: what is written (`workspace_bytes`: the kind's own count) overlaps nothing that is read and no other
	// output. `ranges` comes with three free places in front of what the kind reads: the three outputs every kind has are stated here.
	template<class desc_type, size_t count>
	aclhip_status check_compress_ranges(aclhip_context* context, const char* kind, const desc_type& desc, uint64_t workspace_bytes, uint32_t num_instances, const void* blobs,
		uint64_t blob_stride_bytes, const aclhip_compress_result* results, byte_range (&ranges)[count])
	{
		if (desc.max_tracks == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a %s desc of 0 max_tracks", kind);
		const unsigned __int128 n = num_instances;
		ranges[0] = { "the blob rows", blobs, n * blob_stride_bytes };
		ranges[1] = { "the compress results", results, n * sizeof(aclhip_compress_result) };
		ranges[2] = { "the workspace", desc.workspace, workspace_bytes };
		return check_no_overlap(context, ranges, 3, ranges + 3, count - 3);
	}

	// The shapes of a compressor's launches. They come from the arguments alone -- the handles live on the device --: the analysis takes
	// max_tracks waves per instance (an array holds at most 0xFFFF tracks), the stream a wave per k_compress_dwords_per_lane * 64 dwords
	// of a row, the per-instance kernels a wave per instance.
	struct compress_launch_shape
	{
		static constexpr uint32_t block_size = k_compress_waves_per_block * k_wave_size;
		uint32_t waves_per_instance;		// the stream's
		uint32_t instance_blocks, stream_blocks;
		dim3 track_blocks;					// (tracks, instances)
		int phases;							// measurement knob: only the first k launches -- what each phase costs (tools/scalar_compress.py, tools/transform_compress.py, tools/compress_tracks.py)
	};
	compress_launch_shape compress_launch_shape_of(uint32_t num_instances, uint32_t max_tracks, uint64_t blob_stride_bytes, const char* phases_knob_name)
	{
		compress_launch_shape shape;
		shape.waves_per_instance = waves_per_instance_of(std::min<uint64_t>(blob_stride_bytes, uint64_t(1) << 32) / 4, uint64_t(k_wave_size) * k_compress_dwords_per_lane, num_instances);
		shape.instance_blocks = (num_instances - 1) / k_compress_waves_per_block + 1;
		shape.stream_blocks = uint32_t((uint64_t(num_instances) * shape.waves_per_instance - 1) / k_compress_waves_per_block + 1);
		shape.track_blocks = dim3((std::min<uint32_t>(max_tracks, 0xFFFFu) - 1) / k_compress_waves_per_block + 1, std::min<uint32_t>(num_instances, 65535u));
		const char* phases_knob = lab_knob(phases_knob_name);		// (the lab library alone reads it, per call)
		shape.phases = phases_knob != nullptr ? std::atoi(phases_knob) : INT_MAX;
		return shape;
	}

	// The front of the entry points behind their checks: the batch of none, the device, the registry lock (shared: see launch_tracks)
	// and the table. `launch(stream)` is the kind's own list of kernels, in stream order: each reads what the one before it left in the
	// workspace. Nothing is uploaded.
	template<class table_type, class launch_function>
	aclhip_status launch_compress(aclhip_context* context, table_type aclhip_context::*table, uint32_t num_instances, void* stream_handle, launch_function launch)
	{
		if (context == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
		if (num_instances == 0)
			return ACLHIP_OK;

		device_guard guard(context->device);
		hipStream_t stream = static_cast<hipStream_t>(stream_handle);
		std::shared_lock<std::shared_mutex> lock(context->mutex);
		if (const aclhip_status status = begin_raw_launch(context, context->*table, stream); status != ACLHIP_OK)
			return status;
		return launch(stream);
	}

	// One launch of that list: a kernel that takes its launch record by value, with its grid and block
	struct compress_phase
	{
		const void* kernel;
		dim3 grid, block;
		const void* record;
		template<class record_type>
		compress_phase(void (*kernel)(record_type), dim3 grid, dim3 block, const record_type& record)
			: kernel(reinterpret_cast<const void*>(kernel)), grid(grid), block(block), record(&record) {}
		void operator()(hipStream_t stream) const
		{
			void* arguments[] = { const_cast<void*>(record) };
			(void)hipLaunchKernel(kernel, grid, block, arguments, 0, stream);		// (what it returns is what hipGetLastError() gives next)
		}
	};

	// The first `phases` (compress_launch_shape::phases) of a call's launches, in stream order, each asked for its error. The first one
	// always runs: a knob below 1 counts as 1.
	aclhip_status launch_compress_phases(aclhip_context* context, hipStream_t stream, int phases, const compress_phase* launches, int count)
	{
		for (int k = 0; k < count && k < std::max(phases, 1); ++k)
		{
			launches[k](stream);
			ACLHIP_CHECK_HIP(context, hipGetLastError());
		}
		return ACLHIP_OK;
	}

	// ---- the scalar compressor ---------------------------------------------------------------------------------------------------------

	aclhip_status check_scalar_compress(aclhip_context* context, const aclhip_raw_scalar_tracks* raws, uint32_t num_instances, const aclhip_scalar_compress_desc* desc,
		const void* blobs, uint64_t blob_stride_bytes, const aclhip_compress_result* results)
	{
		if (const aclhip_status status = check_compress_buffers(context, "scalar compress", "raw scalar track", raws, desc, blobs, blob_stride_bytes, results); status != ACLHIP_OK)
			return status;
		if (const aclhip_status status = check_compress_settings(context, "scalar compress", *desc, ACLHIP_COMPRESS_OPTIMIZE_LOOPS); status != ACLHIP_OK)
			return status;
		if (desc->track_precisions != nullptr && desc->num_track_precisions == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "track_precisions with a count of 0");
		byte_range ranges[] =
		{
			{}, {}, {},
			{ "the raw scalar track handles", raws, (unsigned __int128)num_instances * sizeof(aclhip_raw_scalar_tracks) },
			{ "the track precisions", desc->track_precisions, desc->track_precisions != nullptr ? (unsigned __int128)desc->num_track_precisions * sizeof(float) : 0 },
		};
		return check_compress_ranges(context, "scalar compress", *desc, aclhip_scalar_compress_workspace_bytes(num_instances, desc->max_tracks), num_instances, blobs, blob_stride_bytes, results, ranges);
	}
}

// The five launches
extern "C" aclhip_status aclhip_compress_raw_scalar_tracks_batch(aclhip_context* context, const aclhip_raw_scalar_tracks* raws, uint32_t num_instances,
	const aclhip_scalar_compress_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
{
	const aclhip_status status = check_scalar_compress(context, raws, num_instances, desc, blobs, blob_stride_bytes, results);
	if (status != ACLHIP_OK)
		return status;
	return launch_compress(context, &aclhip_context::raw_scalar_tracks, num_instances, stream_handle, [&](hipStream_t stream) -> aclhip_status
	{
		const compress_launch_shape shape = compress_launch_shape_of(num_instances, desc->max_tracks, blob_stride_bytes, "ACLHIP_SCALAR_COMPRESS_PHASES");
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
		launch.instances = reinterpret_cast<compress_instance*>(workspace);
		launch.tracks = reinterpret_cast<scalar_compress_track*>(workspace + uint64_t(num_instances) * sizeof(compress_instance));
		launch.animated = reinterpret_cast<scalar_compress_animated*>(reinterpret_cast<uint8_t*>(launch.tracks) + uint64_t(num_instances) * desc->max_tracks * sizeof(scalar_compress_track));
		launch.blobs = static_cast<uint8_t*>(blobs);
		launch.blob_stride_bytes = blob_stride_bytes;
		launch.results = reinterpret_cast<uint2*>(results);
		launch.waves_per_instance = shape.waves_per_instance;
		launch.rejected_count = context->d_rejected;
		const compress_hash_launch hash_launch = { launch.instances, num_instances, launch.blobs, blob_stride_bytes };

		const dim3 block(shape.block_size);
		const compress_phase phases[] =
		{
			{ scalar_compress_prepare_kernel, dim3(shape.instance_blocks), block, launch },
			{ scalar_compress_analyze_kernel, shape.track_blocks, block, launch },
			{ scalar_compress_layout_kernel, dim3(shape.instance_blocks), block, launch },
			{ scalar_compress_write_kernel, dim3(shape.stream_blocks), block, launch },
			{ compress_hash_kernel, dim3(num_instances), dim3(k_wave_size), hash_launch },
		};
		return launch_compress_phases(context, stream, shape.phases, phases, 5);
	});
}
