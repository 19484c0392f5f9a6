// host_track_maps.inl -- part of aclhip.hip (one translation unit; included there, in this order, not compiled on its own).
// Host side: track maps (track_writer::write_*(track_index, value), core/track_writer.h: the writer chooses the destination) -- what
// registration checks, the record and its image; the handles are a handle_table's (host_context.inl) -- and the mapped pose launch.

namespace
{
	// What registration checks; `first_bad` names the first offending track
	bool check_track_map(const uint32_t* track_to_slot, uint32_t num_tracks, uint32_t num_slots, aclhip_track_map_info& info, std::vector<uint32_t>* out_unmapped,
		char* message, size_t capacity)
	{
		const auto say = [&](const char* format, uint32_t a, uint32_t b, uint32_t c)
		{
			if (message != nullptr && capacity != 0)
				std::snprintf(message, capacity, format, a, b, c);
			return false;
		};
		if (message != nullptr && capacity != 0)
			message[0] = '\0';
		std::memset(&info, 0, sizeof(info));
		if (track_to_slot == nullptr)
			return say("null track_to_slot", 0, 0, 0);
		if (num_tracks == 0 || num_slots == 0)
			return say("a track map of %u tracks into %u slots", num_tracks, num_slots, 0);

		std::vector<uint32_t> owner(num_slots, ACLHIP_TRACK_DROPPED);		// slot -> the track mapped to it
		info.num_tracks = num_tracks;
		info.num_slots = num_slots;
		info.is_order_preserving = 1;
		info.is_identity = num_tracks == num_slots ? 1u : 0u;
		uint32_t previous_slot = 0;
		for (uint32_t track = 0; track < num_tracks; ++track)
		{
			const uint32_t slot = track_to_slot[track];
			if (slot != track)
				info.is_identity = 0;
			if (slot == ACLHIP_TRACK_DROPPED)
			{
				info.num_dropped++;
				continue;
			}
			if (slot >= num_slots)
				return say("track %u maps to slot %u of %u", track, slot, num_slots);
			if (owner[slot] != ACLHIP_TRACK_DROPPED)
				return say("track %u maps to slot %u, which track %u maps to already", track, slot, owner[slot]);
			owner[slot] = track;
			if (info.num_mapped != 0 && slot < previous_slot)
				info.is_order_preserving = 0;
			previous_slot = slot;
			info.num_mapped++;
		}
		info.num_unmapped_slots = num_slots - info.num_mapped;
		if (out_unmapped != nullptr)
		{
			// the tail of the device image: the sorted unmapped slots, then slot -> track (ACLHIP_TRACK_DROPPED: none)
			out_unmapped->clear();
			for (uint32_t slot = 0; slot < num_slots; ++slot)
				if (owner[slot] == ACLHIP_TRACK_DROPPED)
					out_unmapped->push_back(slot);
			out_unmapped->insert(out_unmapped->end(), owner.begin(), owner.end());
		}
		return true;
	}

	// the mapped kernels: a function of its own (pose_kernel_of's names are an inventory the path-knob tests hold to the oracle one by one)
	typedef void (*mapped_pose_kernel)(const device_clip*, uint32_t, const uint32_t*, const float*, uint32_t, uint32_t, decode_params, uint8_t*, uint64_t, uint32_t, unsigned long long*, mapped_launch);

	mapped_pose_kernel mapped_pose_kernel_of(const aclhip_context* context, const decode_params& params)
	{
		const bool any_settings = params.standard_defaults == 0 || params.per_track_rounding != 0 || context->force_generic_kernel;
		return any_settings ? decompress_tracks_mapped_any_settings_kernel : decompress_tracks_mapped_kernel;
	}
}

extern "C" aclhip_status aclhip_check_track_map(const uint32_t* track_to_slot, uint32_t num_tracks, uint32_t num_slots, aclhip_track_map_info* out_info,
	char* message, uint32_t message_capacity)
{
	return guarded(static_cast<aclhip_context*>(nullptr), [&]() -> aclhip_status
	{
		aclhip_track_map_info info;
		const bool valid = check_track_map(track_to_slot, num_tracks, num_slots, info, nullptr, message, message_capacity);
		if (valid && out_info != nullptr)
			*out_info = info;
		return valid ? ACLHIP_OK : ACLHIP_ERROR_INVALID_ARGUMENT;
	});
}

extern "C" aclhip_status aclhip_register_track_map(aclhip_context* context, const uint32_t* track_to_slot, uint32_t num_tracks, uint32_t num_slots, aclhip_track_map* out_map)
{
	if (context == nullptr || out_map == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	*out_map = 0;
	return guarded(context, [&]() -> aclhip_status
	{
		// (everything that needs no device first: a refused map makes no HIP call)
		aclhip_track_map_info info;
		std::vector<uint32_t> image;
		char message[256];
		if (!check_track_map(track_to_slot, num_tracks, num_slots, info, &image, message, sizeof(message)))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s", message);
		image.insert(image.begin(), track_to_slot, track_to_slot + num_tracks);		// track_to_slot[num_tracks] | unmapped slots, ascending | slot_to_track[num_slots]

		std::lock_guard<std::shared_mutex> lock(context->mutex);
		device_guard guard(context->device);
		collect_retired(context, false);

		uint32_t slot;
		if (const aclhip_status status = take_handle(context, context->track_maps, slot); status != ACLHIP_OK)
			return status;

		// (a piece of a clip slab, uploaded on the context's copy stream: no allocation call and no copy that would stall the device)
		uint8_t* d_image = allocate_clip_memory(context, image.size() * sizeof(uint32_t));
		if (d_image == nullptr)
		{
			context->track_maps.give_back(slot);
			return fail(context, ACLHIP_ERROR_OUT_OF_MEMORY, "allocating %zu bytes for the track map failed", image.size() * sizeof(uint32_t));
		}
		device_track_map record;
		std::memset(&record, 0, sizeof(record));
		record.image = reinterpret_cast<const uint32_t*>(d_image);
		record.num_tracks = num_tracks;
		record.num_slots = num_slots;
		record.num_unmapped = info.num_unmapped_slots;
		record.flags = (info.is_identity != 0 ? 1u : 0u) | (info.is_order_preserving != 0 ? 2u : 0u);
		size_t staging_used = 0;
		// the image first, the record that publishes it behind it
		if (!stage_upload(context, d_image, image.data(), image.size() * sizeof(uint32_t), staging_used)
			|| !publish_handle(context, context->track_maps, slot, record, staging_used, info, d_image))
		{
			free_clip_memory(context, d_image);
			context->track_maps.give_back(slot);
			return fail(context, ACLHIP_ERROR_DEVICE, "uploading the track map failed");
		}
		*out_map = slot;
		return ACLHIP_OK;
	});
}

extern "C" aclhip_status aclhip_unregister_track_map(aclhip_context* context, aclhip_track_map map)
{
	if (context == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return unregister_handle(context, context->track_maps, map);
}

extern "C" aclhip_status aclhip_get_track_map_info(const aclhip_context* context, aclhip_track_map map, aclhip_track_map_info* out_info)
{
	if (context == nullptr || out_info == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return get_handle_info(context, context->track_maps, map, out_info);
}

extern "C" aclhip_status aclhip_decompress_tracks_batch_mapped(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_output_desc* output, const aclhip_track_mapping* mapping, void* poses, uint64_t pose_stride_bytes, void* stream_handle)
{
	aclhip_status status = check_batch_arguments(context, clips, sample_times, num_instances, poses, pose_stride_bytes);
	if (status != ACLHIP_OK)
		return status;
	if (mapping == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null track mapping");
	if (mapping->map == 0 && mapping->instance_maps == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a track mapping names a map or a list of maps");
	if (mapping->fill_unmapped > 1)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "fill_unmapped is 0 or 1");
	if (mapping->fill_unmapped != 0 && mapping->fill_pose == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "fill_unmapped without a fill_pose");
	if ((reinterpret_cast<uintptr_t>(mapping->fill_pose) & 15u) != 0)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "fill_pose must be 16 byte aligned");
	if (num_instances == 0)
		return ACLHIP_OK;

	decode_params device_params;
	status = resolve_params(context, params, device_params);
	if (status == ACLHIP_OK)
		status = apply_output_desc(context, output, device_params);
	if (status != ACLHIP_OK)
		return status;

	device_guard guard(context->device);
	hipStream_t stream = static_cast<hipStream_t>(stream_handle);
	std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
	if (context->track_maps.d_records == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no track map was ever registered with this context");
	note_launch_stream(context, stream);

	// shaped like the unmapped launch: one wave per (instance, pose window), the one-shot grid
	const pose_launch_shape shape = pose_launch_shape_of(context, device_params.layout, pose_stride_bytes);
	const uint64_t num_waves = uint64_t(num_instances) * shape.windows_per_instance;
	if (num_waves > 0xFFFFFFFFull - k_waves_per_block)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "batch too large: %u instances x %u pose windows", num_instances, shape.windows_per_instance);
	const uint32_t num_blocks = uint32_t((num_waves + k_waves_per_block - 1) / k_waves_per_block);
	const size_t lds_bytes = size_t(shape.lds_quads_per_wave) * 16 * k_waves_per_block;

	mapped_launch launch;
	launch.maps = context->track_maps.d_records;
	launch.num_maps = ACLHIP_MAX_TRACK_MAPS;
	launch.map = mapping->map;
	launch.instance_maps = mapping->instance_maps;
	launch.fill_pose = mapping->fill_unmapped != 0 ? static_cast<const uint8_t*>(mapping->fill_pose) : nullptr;
	hipLaunchKernelGGL(mapped_pose_kernel_of(context, device_params), dim3(num_blocks), dim3(k_block_size), lds_bytes, stream,
		context->d_clips, context->d_clips_capacity, clips, sample_times, num_instances, shape.windows_per_instance, device_params,
		static_cast<uint8_t*>(poses), pose_stride_bytes, shape.lds_quads_per_wave, context->d_rejected, launch);
	ACLHIP_CHECK_HIP(context, hipGetLastError());
	return ACLHIP_OK;
}
