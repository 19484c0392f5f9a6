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

namespace
{
	// The registration of a raw array of either kind, behind its checks: a handle, the image -- a piece of a clip slab, uploaded on the
	// context's copy stream as the caller laid it out: no copy that would stall the device -- and the record that publishes it behind it.
	// `record` comes filled in but for `samples`.
	template<class table_type, class info_type>
	aclhip_status register_raw_array(aclhip_context* context, table_type& table, const void* samples, size_t image_bytes, typename table_type::record record,
		const info_type& info, uint32_t* out_raw)
	{
		return guarded(context, [&]() -> aclhip_status
		{
			std::lock_guard<std::shared_mutex> lock(context->mutex);
			device_guard guard(context->device);
			collect_retired(context, false);

			uint32_t slot;
			if (const aclhip_status status = take_handle(context, table, slot); status != ACLHIP_OK)
				return status;

			uint8_t* d_image = allocate_clip_memory(context, image_bytes);
			if (d_image == nullptr)
			{
				table.give_back(slot);
				return fail(context, ACLHIP_ERROR_OUT_OF_MEMORY, "allocating %zu bytes for the %s failed", image_bytes, table.noun);
			}
			record.samples = reinterpret_cast<decltype(record.samples)>(d_image);
			size_t staging_used = 0;
			if (!stage_upload(context, d_image, samples, image_bytes, staging_used) || !publish_handle(context, table, slot, record, staging_used, info, d_image))
			{
				free_clip_memory(context, d_image);
				table.give_back(slot);
				return fail(context, ACLHIP_ERROR_DEVICE, "uploading the %s failed", table.noun);
			}
			*out_raw = slot;
			return ACLHIP_OK;
		});
	}
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
	device_raw_tracks record;
	std::memset(&record, 0, sizeof(record));
	record.num_tracks = num_tracks;
	record.num_samples = num_samples;
	record.sample_rate = sample_rate;
	record.duration = info.duration;
	record.looping_policy = looping_policy;
	return register_raw_array(context, context->raw_tracks, samples, size_t(num_samples) * num_tracks * 48, record, info, out_raw);
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
	// ---- sampling a batch of raw arrays of either kind (the three sampling launches) -----------------------------------------------------

	// What tells the three launches apart in their argument checks
	struct raw_sample_kind
	{
		const char* handles;			// "raw track": null raw track handles, the pose rows overlap the raw track handles
		const char* row;				// "pose": null pose buffer, the pose rows overlap the sample times
		uint32_t alignment;				// of the buffer and of its stride, in bytes
		bool refuses_zero_stride;
		const char* alignment_message;
		uint32_t handle_bytes;
		bool has_track_indices;			// the single-track form
	};
	constexpr raw_sample_kind k_raw_tracks_sample = { "raw track", "pose", 16, false, "pose buffer and stride must be 16 byte aligned", sizeof(aclhip_raw_tracks), false };

	// What a sampling launch checks of its arguments before any device call; every refusal leaves a message, with or without a context
	aclhip_status check_raw_sample(aclhip_context* context, const raw_sample_kind& kind, const void* raws, const float* sample_times, const uint32_t* track_indices,
		uint32_t num_instances, const aclhip_raw_sample_desc& desc, const void* rows, uint64_t stride_bytes)
	{
		if (raws == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null %s handles", kind.handles);
		if (sample_times == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null sample times");
		if (kind.has_track_indices && track_indices == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null track indices");
		if (rows == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null %s buffer", kind.row);
		if (((reinterpret_cast<uintptr_t>(rows) | stride_bytes) & (kind.alignment - 1u)) != 0 || (kind.refuses_zero_stride && stride_bytes == 0))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s", kind.alignment_message);
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
		const auto overlap = [&](const void* array, uint64_t element_bytes) { return array != nullptr && pose_ranges_overlap(rows, stride_bytes, array, element_bytes, num_instances); };
		if (overlap(raws, kind.handle_bytes))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the %s rows overlap the %s handles", kind.row, kind.handles);
		if (overlap(sample_times, sizeof(float)))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the %s rows overlap the sample times", kind.row);
		if (kind.has_track_indices && overlap(track_indices, sizeof(uint32_t)))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the %s rows overlap the track indices", kind.row);
		if (overlap(desc.instance_rounding_policies, 1))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the %s rows overlap the instance rounding policies", kind.row);
		if (overlap(desc.rows, sizeof(uint32_t)))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the %s rows overlap the row list", kind.row);
		// (the table's size does not follow the batch. Rows of a stride of 0 are a point, as they are to the checks above: inside the table, it overlaps)
		if (desc.track_rounding_policies != nullptr && num_instances != 0
			&& byte_ranges_meet(rows, (unsigned __int128)stride_bytes * num_instances, desc.track_rounding_policies, desc.num_track_rounding_policies))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the %s rows overlap the track rounding policies", kind.row);
		return ACLHIP_OK;
	}

	// The front of the three launches: a NULL desc, the checks -- they need no device and come first --, the batch of none, the device.
	// `launch(desc)` is the kind's own.
	template<class launch_function>
	aclhip_status sample_raw(aclhip_context* context, const raw_sample_kind& kind, const void* raws, const float* sample_times, const uint32_t* track_indices,
		uint32_t num_instances, const aclhip_raw_sample_desc* desc, const void* rows, uint64_t stride_bytes, launch_function launch)
	{
		aclhip_raw_sample_desc local = {};		// NULL: ROUND_NONE, row i
		if (desc != nullptr)
			local = *desc;
		const aclhip_status status = check_raw_sample(context, kind, raws, sample_times, track_indices, num_instances, local, rows, stride_bytes);
		if (status != ACLHIP_OK)
			return status;
		if (context == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
		if (num_instances == 0)
			return ACLHIP_OK;

		device_guard guard(context->device);
		return launch(local);
	}

	// How a launch that reads one of the two tables begins, under the registry lock (its caller holds it shared: see launch_tracks)
	template<class table_type>
	aclhip_status begin_raw_launch(aclhip_context* context, const table_type& table, hipStream_t stream)
	{
		if (table.d_records == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no %s was ever registered with this context", table.noun);
		note_launch_stream(context, stream);
		return ACLHIP_OK;
	}

	// What the sampling kernels' arguments (raw_sample_launch, raw_scalar_sample_launch) have in common; the rows and the shape are the caller's
	template<class launch_type, class table_type>
	launch_type raw_sample_launch_of(aclhip_context* context, const table_type& table, const uint32_t* raws, const float* sample_times, uint32_t num_instances,
		const aclhip_raw_sample_desc& desc)
	{
		launch_type launch = {};
		launch.arrays = table.d_records;
		launch.num_arrays = table_type::capacity;
		launch.num_instances = num_instances;
		launch.raws = raws;
		launch.sample_times = sample_times;
		launch.rows = desc.rows;
		launch.instance_rounding_policies = desc.instance_rounding_policies;
		launch.track_rounding_policies = desc.track_rounding_policies;
		launch.num_track_rounding_policies = desc.track_rounding_policies != nullptr ? desc.num_track_rounding_policies : 0u;
		launch.rounding_policy = desc.rounding_policy;
		launch.waves_per_instance = 1;
		launch.rejected_count = context->d_rejected;
		return launch;
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
		if (const aclhip_status status = begin_raw_launch(context, context->raw_tracks, stream); status != ACLHIP_OK)
			return status;

		raw_sample_launch launch = raw_sample_launch_of<raw_sample_launch>(context, context->raw_tracks, raws, sample_times, num_instances, desc);
		launch.poses = static_cast<uint8_t*>(poses);
		launch.pose_stride_bytes = pose_stride_bytes;
		// (an array holds at most 0xFFFF tracks)
		const uint64_t row_quads = std::min<uint64_t>(pose_stride_bytes / 16, uint64_t(0xFFFFu) * 3);
		launch.waves_per_instance = waves_per_instance_of(row_quads, uint64_t(k_wave_size) * k_raw_sample_quads_per_lane, num_instances);
		// measurement knob: the waves that share an instance, 1 to one per 64 quads (how the shape above was chosen)
		static const uint32_t forced_waves = []() { const char* value = lab_knob("ACLHIP_RAW_SAMPLE_WAVES"); return value != nullptr ? uint32_t(std::max(0L, std::atol(value))) : 0u; }();
		if (forced_waves != 0)
			launch.waves_per_instance = std::min(waves_per_instance_of(row_quads, k_wave_size, num_instances), forced_waves);

		const uint64_t num_waves = uint64_t(num_instances) * launch.waves_per_instance;
		const uint32_t num_blocks = uint32_t((num_waves + k_raw_sample_waves_per_block - 1) / k_raw_sample_waves_per_block);
		hipLaunchKernelGGL(sample_raw_tracks_kernel, dim3(num_blocks), dim3(k_raw_sample_waves_per_block * k_wave_size), 0, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
		return ACLHIP_OK;
	}
}

// include/aclhip.h states the definition
extern "C" aclhip_status aclhip_sample_raw_tracks_batch(aclhip_context* context, const aclhip_raw_tracks* raws, const float* sample_times, uint32_t num_instances,
	const aclhip_raw_sample_desc* desc, void* poses, uint64_t pose_stride_bytes, void* stream)
{
	return sample_raw(context, k_raw_tracks_sample, raws, sample_times, nullptr, num_instances, desc, poses, pose_stride_bytes, [&](const aclhip_raw_sample_desc& local)
	{
		return launch_raw_sample(context, raws, sample_times, num_instances, local, poses, pose_stride_bytes, static_cast<hipStream_t>(stream));
	});
}
