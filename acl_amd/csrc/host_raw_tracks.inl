// host_raw_tracks.inl -- part of aclhip.hip (one translation unit; included there behind host_skins.inl, not compiled on its own).
// Host side: raw track arrays (an uncompressed clip: acl::track_array_qvvf) -- what registration checks, the record and its image; the
// handles are a handle_table's (host_context.inl) -- and aclhip_sample_raw_tracks_batch (sample_raw_tracks_kernel, kernels_raw_tracks.inl).

namespace
{
	// What registration checks: the shape and the settings, never the values
	bool check_raw_tracks(const void* samples, uint32_t num_tracks, uint32_t num_samples, float sample_rate, uint32_t looping_policy, aclhip_raw_tracks_info& info,
		char* message, size_t capacity)
	{
		const auto say = [&](const char* format, uint32_t a, uint32_t b)
		{
			if (message != nullptr && capacity != 0)
				std::snprintf(message, capacity, format, a, b);
			return false;
		};
		if (message != nullptr && capacity != 0)
			message[0] = '\0';
		std::memset(&info, 0, sizeof(info));
		if (samples == nullptr)
			return say("null samples", 0, 0);
		if (num_tracks == 0)
			return say("a raw track array of %u tracks", num_tracks, 0);
		if (num_tracks > 0xFFFFu)
			return say("%u tracks: a raw track array holds at most 65535", num_tracks, 0);
		if (num_samples == 0)
			return say("a raw track array of %u samples", num_samples, 0);
		if (uint64_t(num_samples) * num_tracks * 48u >= (uint64_t(1) << 31))
			return say("%u samples of %u tracks: a raw track array holds less than 2^31 bytes", num_samples, num_tracks);
		if (!std::isfinite(sample_rate) || !(sample_rate > 0.0f))
		{
			if (message != nullptr && capacity != 0)
				std::snprintf(message, capacity, "a sample rate of %g: it must be finite and above 0", double(sample_rate));
			return false;
		}
		// (track_array::set_looping_policy does not take as_compressed either: there is nothing compressed to ask)
		if (looping_policy == ACLHIP_LOOP_AS_COMPRESSED)
			return say("ACLHIP_LOOP_AS_COMPRESSED: a raw track array is clamped or wrapped", 0, 0);
		if (looping_policy != ACLHIP_LOOP_CLAMP && looping_policy != ACLHIP_LOOP_WRAP)
			return say("unknown looping policy %u", looping_policy, 0);

		// track_array::get_finite_duration (track_array.impl.h:113-124) through the clips' own function
		tracks_header header = {};
		header.num_samples = num_samples;
		header.sample_rate = sample_rate;
		info.num_tracks = num_tracks;
		info.num_samples = num_samples;
		info.sample_rate = sample_rate;
		info.duration = finite_duration(header, uint8_t(looping_policy));
		info.looping_policy = looping_policy;
		return true;
	}
}

extern "C" aclhip_status aclhip_check_raw_tracks(const void* samples, uint32_t num_tracks, uint32_t num_samples, float sample_rate, uint32_t looping_policy,
	aclhip_raw_tracks_info* out_info, char* message, uint32_t message_capacity)
{
	aclhip_raw_tracks_info info;
	const bool valid = check_raw_tracks(samples, num_tracks, num_samples, sample_rate, looping_policy, info, message, message_capacity);
	if (valid && out_info != nullptr)
		*out_info = info;
	return valid ? ACLHIP_OK : ACLHIP_ERROR_INVALID_ARGUMENT;
}

extern "C" aclhip_status aclhip_register_raw_tracks(aclhip_context* context, const void* samples, uint32_t num_tracks, uint32_t num_samples, float sample_rate,
	uint32_t looping_policy, aclhip_raw_tracks* out_raw)
{
	if (out_raw == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null out_raw");
	*out_raw = 0;
	// (everything that needs no device first: a refused array makes no HIP call)
	aclhip_raw_tracks_info info;
	char message[256];
	if (!check_raw_tracks(samples, num_tracks, num_samples, sample_rate, looping_policy, info, message, sizeof(message)))
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s", message);
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	return guarded(context, [&]() -> aclhip_status
	{
		const size_t image_bytes = size_t(num_samples) * num_tracks * 48;

		std::lock_guard<std::shared_mutex> lock(context->mutex);
		device_guard guard(context->device);
		collect_retired(context, false);

		uint32_t slot;
		if (const aclhip_status status = take_handle(context, context->raw_tracks, slot); status != ACLHIP_OK)
			return status;

		// (a piece of a clip slab, uploaded on the context's copy stream: no copy that would stall the device)
		uint8_t* d_image = allocate_clip_memory(context, image_bytes);
		if (d_image == nullptr)
		{
			context->raw_tracks.give_back(slot);
			return fail(context, ACLHIP_ERROR_OUT_OF_MEMORY, "allocating %zu bytes for the raw track array failed", image_bytes);
		}
		device_raw_tracks record;
		std::memset(&record, 0, sizeof(record));
		record.samples = reinterpret_cast<const f32x4*>(d_image);
		record.num_tracks = num_tracks;
		record.num_samples = num_samples;
		record.sample_rate = sample_rate;
		record.duration = info.duration;
		record.looping_policy = looping_policy;
		size_t staging_used = 0;
		// the image first, as the caller laid it out, and the record that publishes it behind it
		if (!stage_upload(context, d_image, samples, image_bytes, staging_used)
			|| !publish_handle(context, context->raw_tracks, slot, record, staging_used, info, d_image))
		{
			free_clip_memory(context, d_image);
			context->raw_tracks.give_back(slot);
			return fail(context, ACLHIP_ERROR_DEVICE, "uploading the raw track array failed");
		}
		*out_raw = slot;
		return ACLHIP_OK;
	});
}

extern "C" aclhip_status aclhip_unregister_raw_tracks(aclhip_context* context, aclhip_raw_tracks raw)
{
	if (context == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return unregister_handle(context, context->raw_tracks, raw);
}

extern "C" aclhip_status aclhip_get_raw_tracks_info(const aclhip_context* context, aclhip_raw_tracks raw, aclhip_raw_tracks_info* out_info)
{
	if (context == nullptr || out_info == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return get_handle_info(context, context->raw_tracks, raw, out_info);
}

namespace
{
	// ---- sampling a batch of raw track arrays (aclhip_sample_raw_tracks_batch; sample_raw_tracks_kernel) ---------------------------------

	// What aclhip_sample_raw_tracks_batch checks of its arguments before any device call; every refusal leaves a message, with or without a context
	aclhip_status check_raw_sample(aclhip_context* context, const aclhip_raw_tracks* raws, const float* sample_times, uint32_t num_instances, const aclhip_raw_sample_desc& desc,
		const void* poses, uint64_t pose_stride_bytes)
	{
		if (raws == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null raw track handles");
		if (sample_times == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null sample times");
		if (poses == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose buffer");
		if ((pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(poses) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose buffer and stride must be 16 byte aligned");
		if (desc.rounding_policy > ACLHIP_ROUND_PER_TRACK)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown rounding policy %u", uint32_t(desc.rounding_policy));
		if (desc.rounding_policy == ACLHIP_ROUND_PER_TRACK && desc.track_rounding_policies == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "ACLHIP_ROUND_PER_TRACK needs track_rounding_policies");
		if (desc.track_rounding_policies != nullptr && desc.num_track_rounding_policies == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "track_rounding_policies with a count of 0");
		bool reserved_clear = desc.reserved1 == 0 && desc.reserved[0] == 0 && desc.reserved[1] == 0;
		for (const uint8_t byte : desc.reserved0)
			reserved_clear = reserved_clear && byte == 0;
		if (!reserved_clear)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a raw sample desc are 0");
		// the rows are written while every array of the launch is read (with `rows` the output range is still taken as num_instances rows)
		if (pose_ranges_overlap(poses, pose_stride_bytes, raws, sizeof(aclhip_raw_tracks), num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the pose rows overlap the raw track handles");
		if (pose_ranges_overlap(poses, pose_stride_bytes, sample_times, sizeof(float), num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the pose rows overlap the sample times");
		if (desc.instance_rounding_policies != nullptr && pose_ranges_overlap(poses, pose_stride_bytes, desc.instance_rounding_policies, 1, num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the pose rows overlap the instance rounding policies");
		if (desc.rows != nullptr && pose_ranges_overlap(poses, pose_stride_bytes, desc.rows, sizeof(uint32_t), num_instances))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the pose rows overlap the row list");
		if (desc.track_rounding_policies != nullptr && num_instances != 0)
		{
			const uint64_t begin = reinterpret_cast<uintptr_t>(desc.track_rounding_policies), end = begin + desc.num_track_rounding_policies;
			const uint64_t out_begin = reinterpret_cast<uintptr_t>(poses);
			const unsigned __int128 out_end = (unsigned __int128)out_begin + (unsigned __int128)pose_stride_bytes * num_instances;
			if (begin < out_end && out_begin < end)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the pose rows overlap the track rounding policies");
		}
		return ACLHIP_OK;
	}

	// The launch: shaped by its pose rows alone -- a row of pose_stride_bytes holds at most pose_stride_bytes / 16 quads, and a wave takes
	// up to k_raw_sample_quads_per_lane of them per lane in turn; which arrays the instances name is the kernel's business. A wave's scalar
	// prologue (handle, record, seek: three dependent loads) is paid once for 8 KiB of row, not once per KiB: measured on 65 536 x 100
	// and x 300 tracks, a lane per quad (5 and 15 waves per instance) took 1.22 x and 1.26 x the time of one wave looping over the row,
	// and 2 and 4 waves per instance measured like one (profiles/raw_tracks.md). Several waves remain for rows beyond 512 quads, so that a
	// small batch of wide rows still fills the device. The table is filled in under the registry lock; nothing is uploaded.
	aclhip_status launch_raw_sample(aclhip_context* context, const aclhip_raw_tracks* raws, const float* sample_times, uint32_t num_instances, const aclhip_raw_sample_desc& desc,
		void* poses, uint64_t pose_stride_bytes, hipStream_t stream)
	{
		std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
		if (context->raw_tracks.d_records == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no raw track array was ever registered with this context");
		note_launch_stream(context, stream);

		// (an array holds at most 0xFFFF tracks; the wave index of the kernel is 32 bits wide: a batch too large for a lane per quad loops)
		const uint64_t row_quads = std::min<uint64_t>(pose_stride_bytes / 16, uint64_t(0xFFFFu) * 3);
		constexpr uint64_t quads_per_wave = uint64_t(k_wave_size) * k_raw_sample_quads_per_lane;
		uint64_t waves_per_instance = std::max<uint64_t>((row_quads + quads_per_wave - 1) / quads_per_wave, 1);
		// measurement knob: the waves that share an instance, 1 to one per 64 quads (how the shape above was chosen)
		static const uint32_t forced_waves = []() { const char* value = lab_knob("ACLHIP_RAW_SAMPLE_WAVES"); return value != nullptr ? uint32_t(std::max(0L, std::atol(value))) : 0u; }();
		if (forced_waves != 0)
			waves_per_instance = std::min<uint64_t>(std::max<uint64_t>((row_quads + k_wave_size - 1) / k_wave_size, 1), forced_waves);
		waves_per_instance = std::min<uint64_t>(waves_per_instance, std::max<uint64_t>(0xFFFFFFF0ull / num_instances, 1));

		raw_sample_launch launch = {};
		launch.arrays = context->raw_tracks.d_records;
		launch.num_arrays = ACLHIP_MAX_RAW_TRACKS;
		launch.num_instances = num_instances;
		launch.raws = raws;
		launch.sample_times = sample_times;
		launch.rows = desc.rows;
		launch.instance_rounding_policies = desc.instance_rounding_policies;
		launch.track_rounding_policies = desc.track_rounding_policies;
		launch.num_track_rounding_policies = desc.track_rounding_policies != nullptr ? desc.num_track_rounding_policies : 0u;
		launch.rounding_policy = desc.rounding_policy;
		launch.poses = static_cast<uint8_t*>(poses);
		launch.pose_stride_bytes = pose_stride_bytes;
		launch.waves_per_instance = uint32_t(waves_per_instance);
		launch.rejected_count = context->d_rejected;

		const uint64_t num_waves = uint64_t(num_instances) * waves_per_instance;
		const uint32_t num_blocks = uint32_t((num_waves + k_raw_sample_waves_per_block - 1) / k_raw_sample_waves_per_block);
		hipLaunchKernelGGL(sample_raw_tracks_kernel, dim3(num_blocks), dim3(k_raw_sample_waves_per_block * k_wave_size), 0, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
		return ACLHIP_OK;
	}
}

// include/aclhip.h states the definition. The argument checks need no device, come first and leave a message, with or without a context.
extern "C" aclhip_status aclhip_sample_raw_tracks_batch(aclhip_context* context, const aclhip_raw_tracks* raws, const float* sample_times, uint32_t num_instances,
	const aclhip_raw_sample_desc* desc, void* poses, uint64_t pose_stride_bytes, void* stream)
{
	aclhip_raw_sample_desc local = {};		// NULL: ROUND_NONE, row i
	if (desc != nullptr)
		local = *desc;
	const aclhip_status status = check_raw_sample(context, raws, sample_times, num_instances, local, poses, pose_stride_bytes);
	if (status != ACLHIP_OK)
		return status;
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	if (num_instances == 0)
		return ACLHIP_OK;

	device_guard guard(context->device);
	return launch_raw_sample(context, raws, sample_times, num_instances, local, poses, pose_stride_bytes, static_cast<hipStream_t>(stream));
}
