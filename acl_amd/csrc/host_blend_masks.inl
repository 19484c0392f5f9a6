// host_blend_masks.inl -- part of aclhip.hip (one translation unit; included there, in this order, not compiled on its own).
// Host side: blend masks (a weight per skeleton slot) and the masked pose consumers' launch. host_track_maps.inl, one to one.

namespace
{
	// What registration checks; the message names the first offending slot
	bool check_blend_mask(const float* weights, uint32_t num_slots, aclhip_blend_mask_info& info, char* message, size_t capacity)
	{
		const auto say = [&](const char* format, uint32_t a, double b)
		{
			if (message != nullptr && capacity != 0)
				std::snprintf(message, capacity, format, a, b);
			return false;
		};
		if (message != nullptr && capacity != 0)
			message[0] = '\0';
		std::memset(&info, 0, sizeof(info));
		if (weights == nullptr)
			return say("null blend mask weights", 0, 0.0);
		if (num_slots == 0)
			return say("a blend mask of %u slots", num_slots, 0.0);
		if (num_slots > 0xFFFFu)
			return say("%u slots: a blend mask holds at most 65535", num_slots, 0.0);

		info.num_slots = num_slots;
		for (uint32_t slot = 0; slot < num_slots; ++slot)
		{
			const float weight = weights[slot];
			if (!std::isfinite(weight))
				return say("slot %u: its weight is not finite", slot, 0.0);
			if (!(weight >= 0.0f && weight <= 1.0f))
				return say("slot %u: weight %.9g is outside [0, 1]", slot, double(weight));
			info.num_zero += weight == 0.0f ? 1u : 0u;
			info.num_one += weight == 1.0f ? 1u : 0u;
		}
		return true;
	}
}

extern "C" aclhip_status aclhip_check_blend_mask(const float* weights, uint32_t num_slots, aclhip_blend_mask_info* out_info, char* message, uint32_t message_capacity)
{
	return guarded(static_cast<aclhip_context*>(nullptr), [&]() -> aclhip_status
	{
		aclhip_blend_mask_info info;
		const bool valid = check_blend_mask(weights, num_slots, info, message, message_capacity);
		if (valid && out_info != nullptr)
			*out_info = info;
		return valid ? ACLHIP_OK : ACLHIP_ERROR_INVALID_ARGUMENT;
	});
}

extern "C" aclhip_status aclhip_register_blend_mask(aclhip_context* context, const float* weights, uint32_t num_slots, aclhip_blend_mask* out_mask)
{
	if (context == nullptr || out_mask == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	*out_mask = 0;
	return guarded(context, [&]() -> aclhip_status
	{
		// (everything that needs no device first: a refused mask makes no HIP call)
		aclhip_blend_mask_info info;
		char message[256];
		if (!check_blend_mask(weights, num_slots, info, message, sizeof(message)))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s", message);

		std::lock_guard<std::shared_mutex> lock(context->mutex);
		device_guard guard(context->device);
		collect_retired(context, false);

		if (context->d_blend_masks == nullptr)
		{
			// once: the table never moves and never grows (a cleared record is an unknown mask)
			device_blend_mask* table = nullptr;
			ACLHIP_CHECK_HIP(context, hipMalloc(reinterpret_cast<void**>(&table), sizeof(device_blend_mask) * ACLHIP_MAX_BLEND_MASKS));
			hipError_t zeroed = hipMemsetAsync(table, 0, sizeof(device_blend_mask) * ACLHIP_MAX_BLEND_MASKS, context->copy_stream);
			if (zeroed == hipSuccess)
				zeroed = hipStreamSynchronize(context->copy_stream);
			if (zeroed != hipSuccess)
			{
				(void)hipFree(table);
				ACLHIP_CHECK_HIP(context, zeroed);
			}
			context->d_blend_masks = table;
			context->blend_masks.resize(1);		// handle 0: none
		}

		uint32_t slot;
		if (!context->free_blend_mask_slots.empty())
		{
			slot = context->free_blend_mask_slots.back();
			context->free_blend_mask_slots.pop_back();
		}
		else
		{
			if (context->blend_masks.size() >= ACLHIP_MAX_BLEND_MASKS)
				return fail(context, ACLHIP_ERROR_OUT_OF_MEMORY, "the blend mask table holds %u masks", ACLHIP_MAX_BLEND_MASKS - 1);
			slot = uint32_t(context->blend_masks.size());
			context->blend_masks.emplace_back();
		}
		const auto give_back = [&]() { context->free_blend_mask_slots.push_back(slot); };

		// (a piece of a clip slab, uploaded on the context's copy stream: no allocation call and no copy that would stall the device)
		const size_t image_bytes = size_t(num_slots) * sizeof(float);
		uint8_t* d_image = allocate_clip_memory(context, image_bytes);
		if (d_image == nullptr)
		{
			give_back();
			return fail(context, ACLHIP_ERROR_OUT_OF_MEMORY, "allocating %zu bytes for the blend mask failed", image_bytes);
		}
		device_blend_mask record;
		std::memset(&record, 0, sizeof(record));
		record.image = reinterpret_cast<const float*>(d_image);
		record.num_slots = num_slots;
		size_t staging_used = 0;
		// the image first, the record that publishes it behind it (one stream: in order)
		if (!stage_upload(context, d_image, weights, image_bytes, staging_used)
			|| !stage_upload(context, context->d_blend_masks + slot, &record, sizeof(record), staging_used)
			|| !finish_uploads(context))
		{
			free_clip_memory(context, d_image);
			give_back();
			return fail(context, ACLHIP_ERROR_DEVICE, "uploading the blend mask failed");
		}
		aclhip_context::blend_mask_entry& entry = context->blend_masks[slot];
		entry.in_use = true;
		entry.info = info;
		entry.device_memory = d_image;
		*out_mask = slot;
		return ACLHIP_OK;
	});
}

extern "C" aclhip_status aclhip_unregister_blend_mask(aclhip_context* context, aclhip_blend_mask mask)
{
	if (context == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;

	std::lock_guard<std::shared_mutex> lock(context->mutex);
	if (mask == 0 || mask >= context->blend_masks.size() || !context->blend_masks[mask].in_use)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown blend mask handle %u", mask);

	device_guard guard(context->device);
	collect_retired(context, false);
	// stream ordered, nobody waits (aclhip_unregister_track_map): the record is cleared behind the launches already enqueued, the image and
	// the handle are recycled once both have happened
	aclhip_context::retired_item item;
	item.clip_memory = context->blend_masks[mask].device_memory;
	item.blend_mask_slot = mask;
	retire(context, std::move(item), context->d_blend_masks + mask, sizeof(device_blend_mask));
	context->blend_masks[mask] = aclhip_context::blend_mask_entry();
	return ACLHIP_OK;
}

extern "C" aclhip_status aclhip_get_blend_mask_info(const aclhip_context* context, aclhip_blend_mask mask, aclhip_blend_mask_info* out_info)
{
	if (context == nullptr || out_info == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	aclhip_context* mutable_context = const_cast<aclhip_context*>(context);
	std::shared_lock<std::shared_mutex> lock(mutable_context->mutex);
	if (mask == 0 || mask >= context->blend_masks.size() || !context->blend_masks[mask].in_use)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown blend mask handle %u", mask);
	*out_info = context->blend_masks[mask].info;
	return ACLHIP_OK;
}

namespace
{
	// What the masked launches (_masked, _bounds with a masking) check of their masking, and the launch argument made of it
	aclhip_status check_blend_masking(aclhip_context* context, const aclhip_pose_consumers* consumers, const aclhip_blend_masking* masking)
	{
		if (masking->mode > ACLHIP_BLEND_LAYERED)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown blend mode %u", masking->mode);
		if (masking->reserved0 != 0 || masking->reserved[0] != 0 || masking->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a blend masking are 0");
		if (masking->instance_masks == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a blend masking names a list of masks (entries may be 0)");
		if (consumers->num_blend_clips < 2)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "blend masks go with a blend: num_blend_clips is %u", consumers->num_blend_clips);
		return ACLHIP_OK;
	}

	blend_mask_launch blend_mask_launch_of(const aclhip_blend_masking* masking)
	{
		blend_mask_launch launch = {};
		launch.layered = masking->mode == ACLHIP_BLEND_LAYERED ? 1u : 0u;
		launch.instance_masks = masking->instance_masks;
		return launch;
	}
}

extern "C" aclhip_status aclhip_decompress_poses_batch_masked(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping, const aclhip_blend_masking* masking,
	void* poses, uint64_t pose_stride_bytes, void* stream)
{
	aclhip_status status = check_batch_arguments(context, clips, sample_times, num_instances, poses, pose_stride_bytes);
	if (status != ACLHIP_OK)
		return status;
	if (consumers == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null consumers");
	if (mapping == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose mapping");
	if (masking == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null blend masking");
	status = check_blend_masking(context, consumers, masking);
	if (status == ACLHIP_OK)
		status = check_pose_mapping(context, consumers, mapping);
	if (status != ACLHIP_OK)
		return status;
	if (num_instances == 0)
		return ACLHIP_OK;

	decode_params device_params;
	status = resolve_params(context, params, device_params);
	if (status != ACLHIP_OK)
		return status;

	const skeleton_launch launch = skeleton_launch_of(consumers, mapping);
	const blend_mask_launch mask_launch = blend_mask_launch_of(masking);

	device_guard guard(context->device);
	return launch_consumers(context, clips, sample_times, num_instances, device_params, *consumers, poses, pose_stride_bytes, static_cast<hipStream_t>(stream), &launch, &mask_launch);
}

namespace
{
	// What every launch with bounds (_bounds, aclhip_transform_poses_batch) checks of the struct itself
	aclhip_status check_pose_bounds(aclhip_context* context, const aclhip_pose_bounds* bounds)
	{
		if (bounds->bounds == nullptr || (reinterpret_cast<uintptr_t>(bounds->bounds) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the bounds buffer must be set and 16 byte aligned");
		if (bounds->reserved[0] != 0 || bounds->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of pose bounds are 0");
		return ACLHIP_OK;
	}
}

// The launch above, the mapped launch or the unmapped one -- by which of `mapping` and `masking` are set -- with a box per instance
// (include/aclhip.h: aclhip_pose_bounds). The argument checks that need no device come first and leave a message, with or without a context.
extern "C" aclhip_status aclhip_decompress_poses_batch_bounds(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping, const aclhip_blend_masking* masking,
	const aclhip_pose_bounds* bounds, void* poses, uint64_t pose_stride_bytes, void* stream)
{
	if (bounds == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose bounds");
	if (const aclhip_status bounds_status = check_pose_bounds(context, bounds); bounds_status != ACLHIP_OK)
		return bounds_status;
	if (consumers == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null consumers");
	if (consumers->object_space == 0)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose bounds are taken in object space: a local space translation is not a position");
	if (masking != nullptr && mapping == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "blend masks go with a pose mapping");
	// check_batch_arguments without its pose buffer: `poses` may be null here (the bounds alone)
	if (num_instances != 0 && (clips == nullptr || sample_times == nullptr))
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null instance list");
	if ((pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(poses) & 15u) != 0)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose buffer and stride must be 16 byte aligned");
	aclhip_status status = masking != nullptr ? check_blend_masking(context, consumers, masking) : ACLHIP_OK;
	if (status == ACLHIP_OK && mapping != nullptr)
		status = check_pose_mapping(context, consumers, mapping);
	if (status != ACLHIP_OK)
		return status;
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	if (num_instances == 0)
		return ACLHIP_OK;

	decode_params device_params;
	status = resolve_params(context, params, device_params);
	if (status != ACLHIP_OK)
		return status;

	const skeleton_launch launch = mapping != nullptr ? skeleton_launch_of(consumers, mapping) : skeleton_launch{};
	const blend_mask_launch mask_launch = masking != nullptr ? blend_mask_launch_of(masking) : blend_mask_launch{};
	const consumer_bounds_launch bounds_launch = { static_cast<uint8_t*>(bounds->bounds), bounds->bone_flags };

	device_guard guard(context->device);
	return launch_consumers(context, clips, sample_times, num_instances, device_params, *consumers, poses, pose_stride_bytes, static_cast<hipStream_t>(stream),
		mapping != nullptr ? &launch : nullptr, masking != nullptr ? &mask_launch : nullptr, &bounds_launch);
}

namespace
{
	// What the additive launch checks of its layering
	aclhip_status check_additive_layering(aclhip_context* context, const aclhip_pose_consumers* consumers, const aclhip_additive_layering* layering)
	{
		if (layering->instance_weights == nullptr && layering->instance_masks == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "an additive layering names instance_weights or instance_masks (without both it is aclhip_decompress_poses_batch_mapped)");
		if (layering->reserved[0] != 0 || layering->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of an additive layering are 0");
		if (consumers->additive_format == ACLHIP_ADDITIVE_NONE)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "an additive layering goes with an additive format: additive_format is NONE");
		return ACLHIP_OK;
	}
}

// aclhip_decompress_poses_batch_mapped with a strength per (instance, slot) on the additive pose (include/aclhip.h:
// aclhip_additive_layering). The argument checks that need no device come first and leave a message, with or without a context.
extern "C" aclhip_status aclhip_decompress_poses_batch_additive_weighted(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping, const aclhip_additive_layering* layering,
	void* poses, uint64_t pose_stride_bytes, void* stream)
{
	if (layering == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null additive layering");
	if (consumers == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null consumers");
	if (mapping == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose mapping");
	aclhip_status status = check_additive_layering(context, consumers, layering);
	if (status == ACLHIP_OK)
		status = check_pose_mapping(context, consumers, mapping);
	if (status != ACLHIP_OK)
		return status;
	// (check_batch_arguments' refusals, said here as well: it has no message without a context)
	if (num_instances != 0 && (clips == nullptr || sample_times == nullptr || poses == nullptr))
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null instance list or output buffer");
	if ((pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(poses) & 15u) != 0)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose buffer and stride must be 16 byte aligned");
	if (context == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null context");
	status = check_batch_arguments(context, clips, sample_times, num_instances, poses, pose_stride_bytes);
	if (status != ACLHIP_OK)
		return status;
	if (num_instances == 0)
		return ACLHIP_OK;

	decode_params device_params;
	status = resolve_params(context, params, device_params);
	if (status != ACLHIP_OK)
		return status;

	const skeleton_launch launch = skeleton_launch_of(consumers, mapping);
	additive_strength_launch strength_launch = {};
	strength_launch.instance_weights = layering->instance_weights;
	strength_launch.instance_masks = layering->instance_masks;

	device_guard guard(context->device);
	return launch_consumers(context, clips, sample_times, num_instances, device_params, *consumers, poses, pose_stride_bytes, static_cast<hipStream_t>(stream), &launch, nullptr, nullptr, &strength_launch);
}
