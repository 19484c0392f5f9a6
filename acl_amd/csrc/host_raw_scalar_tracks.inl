// host_raw_scalar_tracks.inl -- part of aclhip.hip (one translation unit; included there behind host_raw_tracks.inl, not compiled on its own).
// Host side: raw scalar track arrays (an uncompressed curve set: acl::track_array of float1f .. vector4f) -- what registration checks, the
// record and its image; the handles are a handle_table's (host_context.inl) --, aclhip_sample_raw_scalar_tracks_batch,
// aclhip_sample_raw_scalar_track_batch and aclhip_measure_scalar_error_batch (kernels_raw_scalar_tracks.inl).

namespace
{
	// acl::track_type8 -> floats per track; 0 for qvvf and everything unknown
	uint32_t raw_scalar_components_of(uint32_t track_type)
	{
		return track_type <= 3 ? track_type + 1 : (track_type == 4 ? 4u : 0u);
	}

	// What registration checks: the shape and the settings, never the values
	bool check_raw_scalar_tracks(const void* samples, uint32_t track_type, uint32_t num_tracks, uint32_t num_samples, float sample_rate, uint32_t looping_policy,
		aclhip_raw_scalar_tracks_info& info, char* message, size_t capacity)
	{
		if (message != nullptr && capacity != 0)
			message[0] = '\0';
		std::memset(&info, 0, sizeof(info));
		const auto say = [&](const char* text)
		{
			if (message != nullptr && capacity != 0)
				std::snprintf(message, capacity, "%s", text);
			return false;
		};
		if (track_type == 12)
			return say("track type 12 (qvvf): a transform array is a raw track array (aclhip_register_raw_tracks)");
		const uint32_t num_components = raw_scalar_components_of(track_type);
		if (num_components == 0)
		{
			if (message != nullptr && capacity != 0)
				std::snprintf(message, capacity, "unknown track type %u", track_type);
			return false;
		}
		// the shape and the settings are the qvvf array's; its size limit is restated for C floats per track
		aclhip_raw_tracks_info shape;
		if (!check_raw_tracks(samples, num_tracks, 1, sample_rate, looping_policy, shape, message, capacity))
			return false;
		if (num_samples == 0)
			return say("a raw scalar track array of 0 samples");
		if (uint64_t(num_samples) * num_tracks * num_components * 4u >= (uint64_t(1) << 31))
		{
			if (message != nullptr && capacity != 0)
				std::snprintf(message, capacity, "%u samples of %u tracks of %u floats: a raw scalar track array holds less than 2^31 bytes", num_samples, num_tracks, num_components);
			return false;
		}

		tracks_header header = {};
		header.num_samples = num_samples;
		header.sample_rate = sample_rate;
		info.num_tracks = num_tracks;
		info.num_samples = num_samples;
		info.sample_rate = sample_rate;
		info.duration = finite_duration(header, uint8_t(looping_policy));
		info.looping_policy = looping_policy;
		info.track_type = track_type;
		info.num_components = num_components;
		return true;
	}
}

extern "C" aclhip_status aclhip_check_raw_scalar_tracks(const void* samples, uint32_t track_type, uint32_t num_tracks, uint32_t num_samples, float sample_rate,
	uint32_t looping_policy, aclhip_raw_scalar_tracks_info* out_info, char* message, uint32_t message_capacity)
{
	aclhip_raw_scalar_tracks_info info;
	const bool valid = check_raw_scalar_tracks(samples, track_type, num_tracks, num_samples, sample_rate, looping_policy, info, message, message_capacity);
	if (valid && out_info != nullptr)
		*out_info = info;
	return valid ? ACLHIP_OK : ACLHIP_ERROR_INVALID_ARGUMENT;
}

extern "C" aclhip_status aclhip_register_raw_scalar_tracks(aclhip_context* context, const void* samples, uint32_t track_type, uint32_t num_tracks, uint32_t num_samples,
	float sample_rate, uint32_t looping_policy, aclhip_raw_scalar_tracks* out_raw)
{
	if (out_raw == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null out_raw");
	*out_raw = 0;
	// (everything that needs no device first: a refused array makes no HIP call)
	aclhip_raw_scalar_tracks_info info;
	char message[256];
	if (!check_raw_scalar_tracks(samples, track_type, num_tracks, num_samples, sample_rate, looping_policy, info, message, sizeof(message)))
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s", message);
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	device_raw_scalar_tracks record;
	std::memset(&record, 0, sizeof(record));
	record.num_tracks = num_tracks;
	record.num_samples = num_samples;
	record.sample_rate = sample_rate;
	record.duration = info.duration;
	record.looping_policy = looping_policy | (track_type << 8);
	record.num_components = info.num_components;
	return register_raw_array(context, context->raw_scalar_tracks, samples, size_t(num_samples) * num_tracks * info.num_components * 4, record, info, out_raw);
}

extern "C" aclhip_status aclhip_unregister_raw_scalar_tracks(aclhip_context* context, aclhip_raw_scalar_tracks raw)
{
	if (context == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return unregister_handle(context, context->raw_scalar_tracks, raw);
}

extern "C" aclhip_status aclhip_get_raw_scalar_tracks_info(const aclhip_context* context, aclhip_raw_scalar_tracks raw, aclhip_raw_scalar_tracks_info* out_info)
{
	if (context == nullptr || out_info == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return get_handle_info(context, context->raw_scalar_tracks, raw, out_info);
}

namespace
{
	// ---- sampling a batch of raw scalar track arrays (both launches; their checks and their front are sample_raw's, host_raw_tracks.inl) ---

	constexpr const char* k_raw_scalar_alignment_message = "the value buffer and its stride must be 4 byte aligned, and the stride is not 0";
	constexpr raw_sample_kind k_raw_scalar_tracks_sample = { "raw scalar track", "value", 4, true, k_raw_scalar_alignment_message, sizeof(aclhip_raw_scalar_tracks), false };
	constexpr raw_sample_kind k_raw_scalar_track_sample = { "raw scalar track", "value", 4, true, k_raw_scalar_alignment_message, sizeof(aclhip_raw_scalar_tracks), true };

	// The launches. The whole-list one is shaped by its rows alone: a row of stride_bytes holds at most stride_bytes / 4 floats, and a wave
	// takes up to k_raw_scalar_elements_per_lane of them per lane (in turns of one float per lane, or of four where the 16 byte path is taken) (launch_raw_sample, host_raw_tracks.inl, says why a wave loops);
	// which arrays the instances name is the kernel's business. The single-track one (`track_indices`) is a thread per request. The table
	// is filled in under the registry lock; nothing is uploaded.
	aclhip_status launch_raw_scalar_sample(aclhip_context* context, const aclhip_raw_scalar_tracks* raws, const float* sample_times, const uint32_t* track_indices,
		uint32_t num_instances, const aclhip_raw_sample_desc& desc, void* values, uint64_t stride_bytes, hipStream_t stream)
	{
		std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
		if (const aclhip_status status = begin_raw_launch(context, context->raw_scalar_tracks, stream); status != ACLHIP_OK)
			return status;

		raw_scalar_sample_launch launch = raw_sample_launch_of<raw_scalar_sample_launch>(context, context->raw_scalar_tracks, raws, sample_times, num_instances, desc);
		launch.track_indices = track_indices;
		launch.values = static_cast<uint8_t*>(values);
		launch.stride_bytes = stride_bytes;
		// measurement knob: the dword path for every row (what the 16 byte path buys: tools/raw_scalar_tracks.py, profiles/raw_scalar_tracks.md)
		static const bool dword_only = []() { const char* value = lab_knob("ACLHIP_RAW_SCALAR_DWORD"); return value != nullptr && value[0] == '1'; }();
		launch.dword_only = dword_only ? 1u : 0u;

		if (track_indices != nullptr)
		{
			constexpr uint32_t block_size = k_raw_scalar_waves_per_block * k_wave_size;
			hipLaunchKernelGGL(sample_raw_scalar_track_kernel, dim3((num_instances + block_size - 1) / block_size), dim3(block_size), 0, stream, launch);
		}
		else
		{
			// (an array holds at most 0xFFFF tracks of 4 floats)
			const uint64_t row_elements = std::min<uint64_t>(stride_bytes / 4, uint64_t(0xFFFFu) * 4);
			launch.waves_per_instance = waves_per_instance_of(row_elements, uint64_t(k_wave_size) * k_raw_scalar_elements_per_lane, num_instances);
			const uint64_t num_waves = uint64_t(num_instances) * launch.waves_per_instance;
			const uint32_t num_blocks = uint32_t((num_waves + k_raw_scalar_waves_per_block - 1) / k_raw_scalar_waves_per_block);
			hipLaunchKernelGGL(sample_raw_scalar_tracks_kernel, dim3(num_blocks), dim3(k_raw_scalar_waves_per_block * k_wave_size), 0, stream, launch);
		}
		ACLHIP_CHECK_HIP(context, hipGetLastError());
		return ACLHIP_OK;
	}
}

// include/aclhip.h states the definitions
extern "C" aclhip_status aclhip_sample_raw_scalar_tracks_batch(aclhip_context* context, const aclhip_raw_scalar_tracks* raws, const float* sample_times, uint32_t num_instances,
	const aclhip_raw_sample_desc* desc, void* values, uint64_t stride_bytes, void* stream)
{
	return sample_raw(context, k_raw_scalar_tracks_sample, raws, sample_times, nullptr, num_instances, desc, values, stride_bytes, [&](const aclhip_raw_sample_desc& local)
	{
		return launch_raw_scalar_sample(context, raws, sample_times, nullptr, num_instances, local, values, stride_bytes, static_cast<hipStream_t>(stream));
	});
}

extern "C" aclhip_status aclhip_sample_raw_scalar_track_batch(aclhip_context* context, const aclhip_raw_scalar_tracks* raws, const float* sample_times, const uint32_t* track_indices,
	uint32_t num_instances, const aclhip_raw_sample_desc* desc, void* values, uint64_t stride_bytes, void* stream)
{
	return sample_raw(context, k_raw_scalar_track_sample, raws, sample_times, track_indices, num_instances, desc, values, stride_bytes, [&](const aclhip_raw_sample_desc& local)
	{
		return launch_raw_scalar_sample(context, raws, sample_times, track_indices, num_instances, local, values, stride_bytes, static_cast<hipStream_t>(stream));
	});
}

namespace
{
	// ---- the scalar track error of two value buffers (aclhip_measure_scalar_error_batch; measure_scalar_error_kernel) ---------------------

	// What the launch checks of its arguments before any device call; every refusal leaves a message, with or without a context
	aclhip_status check_scalar_error(aclhip_context* context, const void* raw_values, uint64_t raw_stride_bytes, const void* lossy_values, uint64_t lossy_stride_bytes,
		uint32_t num_instances, const aclhip_scalar_error_desc* desc, const aclhip_track_error* errors)
	{
		if (desc == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null scalar error desc");
		if (raw_values == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null raw value buffer");
		if (lossy_values == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null lossy value buffer");
		if (errors == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null track error records");
		if (desc->num_tracks == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a scalar error desc of 0 tracks");
		if (desc->num_components < 1 || desc->num_components > 4)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%u components per track: a scalar track has 1 to 4", desc->num_components);
		const uint64_t row_bytes = uint64_t(desc->num_tracks) * desc->num_components * 4u;
		if (row_bytes > raw_stride_bytes || row_bytes > lossy_stride_bytes)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%u tracks of %u floats do not fit the value strides", desc->num_tracks, desc->num_components);
		if ((raw_stride_bytes & 3u) != 0 || (reinterpret_cast<uintptr_t>(raw_values) & 3u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "raw value buffer and stride must be 4 byte aligned");
		if ((lossy_stride_bytes & 3u) != 0 || (reinterpret_cast<uintptr_t>(lossy_values) & 3u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "lossy value buffer and stride must be 4 byte aligned");
		if (desc->track_errors != nullptr && (desc->track_error_stride_bytes == 0 || (desc->track_error_stride_bytes & 3u) != 0 || (reinterpret_cast<uintptr_t>(desc->track_errors) & 3u) != 0
			|| desc->track_error_stride_bytes < uint64_t(desc->num_tracks) * 4u))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "track errors are 4 byte aligned and their stride is a multiple of 4 that holds every track");
		if ((reinterpret_cast<uintptr_t>(errors) & 7u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "track error records must be 8 byte aligned");
		if ((reinterpret_cast<uintptr_t>(desc->worst) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the worst track error record must be 16 byte aligned");
		if (desc->reserved[0] != 0 || desc->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a scalar error desc are 0");

		// raw and lossy are only read and may be the same buffer; what is written overlaps nothing that is read and no other output
		const unsigned __int128 n = num_instances;
		return check_no_overlap(context,
			{
				{ "the track error records", errors, n * sizeof(aclhip_track_error) },
				{ "the track errors", desc->track_errors, desc->track_errors != nullptr ? n * desc->track_error_stride_bytes : 0 },
				{ "the worst record", desc->worst, desc->worst != nullptr ? sizeof(aclhip_track_error_worst) : 0 },
			},
			{ { "the raw value rows", raw_values, n * raw_stride_bytes }, { "the lossy value rows", lossy_values, n * lossy_stride_bytes } });
	}
}

// include/aclhip.h states the definition. The worst record is pose_error_worst_kernel's, on the same stream behind the measure -- the
// only launch of a batch of none. Nothing is uploaded and no table is read: the registry lock is held for the stream's note alone.
extern "C" aclhip_status aclhip_measure_scalar_error_batch(aclhip_context* context, const void* raw_values, uint64_t raw_stride_bytes, const void* lossy_values,
	uint64_t lossy_stride_bytes, uint32_t num_instances, const aclhip_scalar_error_desc* desc, aclhip_track_error* errors, void* stream_handle)
{
	const aclhip_status status = check_scalar_error(context, raw_values, raw_stride_bytes, lossy_values, lossy_stride_bytes, num_instances, desc, errors);
	if (status != ACLHIP_OK)
		return status;
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	if (num_instances == 0 && desc->worst == nullptr)
		return ACLHIP_OK;

	device_guard guard(context->device);
	hipStream_t stream = static_cast<hipStream_t>(stream_handle);
	std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
	note_launch_stream(context, stream);
	if (num_instances != 0)
	{
		scalar_error_launch launch = {};
		launch.raw_values = static_cast<const uint8_t*>(raw_values);
		launch.raw_stride_bytes = raw_stride_bytes;
		launch.lossy_values = static_cast<const uint8_t*>(lossy_values);
		launch.lossy_stride_bytes = lossy_stride_bytes;
		launch.track_errors = reinterpret_cast<uint8_t*>(desc->track_errors);
		launch.track_error_stride_bytes = desc->track_error_stride_bytes;
		launch.errors = reinterpret_cast<pose_error_record*>(errors);
		launch.num_instances = num_instances;
		launch.num_tracks = desc->num_tracks;
		launch.num_components = desc->num_components;
		const uint32_t num_blocks = (num_instances - 1) / k_scalar_error_waves_per_block + 1;
		hipLaunchKernelGGL(measure_scalar_error_kernel, dim3(num_blocks), dim3(k_scalar_error_waves_per_block * k_wave_size), 0, stream, launch);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
	}
	if (desc->worst != nullptr)
	{
		hipLaunchKernelGGL(pose_error_worst_kernel, dim3(1), dim3(k_pose_error_worst_threads), 0, stream, reinterpret_cast<const pose_error_record*>(errors), num_instances,
			reinterpret_cast<u32x4*>(desc->worst));
		ACLHIP_CHECK_HIP(context, hipGetLastError());
	}
	return ACLHIP_OK;
}
