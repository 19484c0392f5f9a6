// host_blend_masks.inl -- part of aclhip.hip (one translation unit; included there, in this order, not compiled on its own).
// Host side: blend masks (a weight per skeleton slot) -- what registration checks, the record and its image; the handles are a
// handle_table's (host_context.inl) -- and the entry points of the masked, the bounds and the additive weighted pose launches.

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

		uint32_t slot;
		if (const aclhip_status status = take_handle(context, context->blend_masks, slot); status != ACLHIP_OK)
			return status;

		// (a piece of a clip slab, uploaded on the context's copy stream: no allocation call and no copy that would stall the device)
		const size_t image_bytes = size_t(num_slots) * sizeof(float);
		uint8_t* d_image = allocate_clip_memory(context, image_bytes);
		if (d_image == nullptr)
		{
			context->blend_masks.give_back(slot);
			return fail(context, ACLHIP_ERROR_OUT_OF_MEMORY, "allocating %zu bytes for the blend mask failed", image_bytes);
		}
		device_blend_mask record;
		std::memset(&record, 0, sizeof(record));
		record.image = reinterpret_cast<const float*>(d_image);
		record.num_slots = num_slots;
		size_t staging_used = 0;
		// the image first, the record that publishes it behind it
		if (!stage_upload(context, d_image, weights, image_bytes, staging_used)
			|| !publish_handle(context, context->blend_masks, slot, record, staging_used, info, d_image))
		{
			free_clip_memory(context, d_image);
			context->blend_masks.give_back(slot);
			return fail(context, ACLHIP_ERROR_DEVICE, "uploading the blend mask failed");
		}
		*out_mask = slot;
		return ACLHIP_OK;
	});
}

extern "C" aclhip_status aclhip_unregister_blend_mask(aclhip_context* context, aclhip_blend_mask mask)
{
	if (context == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return unregister_handle(context, context->blend_masks, mask);
}

extern "C" aclhip_status aclhip_get_blend_mask_info(const aclhip_context* context, aclhip_blend_mask mask, aclhip_blend_mask_info* out_info)
{
	if (context == nullptr || out_info == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return get_handle_info(context, context->blend_masks, mask, out_info);
}

extern "C" aclhip_status aclhip_decompress_poses_batch_masked(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping, const aclhip_blend_masking* masking,
	void* poses, uint64_t pose_stride_bytes, void* stream)
{
	if (mapping == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose mapping");
	if (masking == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null blend masking");
	return launch_pose_consumers(context, clips, sample_times, num_instances, params, consumers, { mapping, masking, nullptr, nullptr }, poses, pose_stride_bytes, stream);
}

// The launch above, the mapped launch or the unmapped one -- by which of `mapping` and `masking` are set -- with a box per instance
// (include/aclhip.h: aclhip_pose_bounds); `poses` may be null (the boxes alone).
extern "C" aclhip_status aclhip_decompress_poses_batch_bounds(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping, const aclhip_blend_masking* masking,
	const aclhip_pose_bounds* bounds, void* poses, uint64_t pose_stride_bytes, void* stream)
{
	if (bounds == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose bounds");
	return launch_pose_consumers(context, clips, sample_times, num_instances, params, consumers, { mapping, masking, bounds, nullptr }, poses, pose_stride_bytes, stream);
}

// aclhip_decompress_poses_batch_mapped with a strength per (instance, slot) on the additive pose (include/aclhip.h: aclhip_additive_layering)
extern "C" aclhip_status aclhip_decompress_poses_batch_additive_weighted(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping, const aclhip_additive_layering* layering,
	void* poses, uint64_t pose_stride_bytes, void* stream)
{
	if (layering == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null additive layering");
	if (mapping == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose mapping");
	return launch_pose_consumers(context, clips, sample_times, num_instances, params, consumers, { mapping, nullptr, nullptr, layering }, poses, pose_stride_bytes, stream);
}
