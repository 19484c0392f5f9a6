// kernels_bone_object.inl -- part of aclhip.hip (one translation unit; included there behind kernels_track.inl, not compiled on its own).
// decompress_bone_object_kernel: single (instance, bone) requests in OBJECT space (aclhip_decompress_track_object_batch,
// aclhip_decompress_bone_object_batch_mapped): one record of the row the object space pose consumers write, without the row.
//
// One wave64 takes 64 consecutive requests, lanes <-> requests, and every lane works its own request from start to end:
//   1. clip handle, sample time, bone in. The clip record as in decompress_track_kernel: on the scalar unit when the wave names ONE
//      clip, gathered four lanes per record otherwise (gather_clip_records, with the record's tail: the hierarchy pointer lives there).
//      Skeleton space: the request's skeleton and map records, 32 bytes each, per lane.
//   2. the seek runs ONCE per request: every ancestor of the bone is sampled at the same time. That, and the bytes written, is what the
//      launch saves over depth(bone) separate single track requests and over the whole-pose route.
//   3. the bone's ancestor chain comes from the hierarchy's PARENT TABLE (one word per transform: parent | depth << 16, appended to the
//      walk schedule image by build_walk_schedule_image -- the schedule itself is in step order and cannot be indexed by bone). The table
//      leads from the bone UP and the product has to run from the root DOWN (fp32 products do not associate), so a lane climbs its chain
//      once per segment of k_bone_chain_levels levels, leaves the segment's transforms in an LDS stack of its own (2 KiB per wave) and
//      then descends through it: one climb for chains of up to 16 transforms (every humanoid), depth / 16 climbs for deeper ones -- no
//      chain is too long, and nothing is sized by the deepest registered hierarchy.
//   4. per level a lane fetches its ancestor's three base pose quads and decodes the animated ones IN THE LANE, kind by kind (a pass per
//      kind that some lane of the wave has animated: up to three passes per level, against the dense (request, kind) packing of
//      decompress_track_requests -- see DESIGN.md 4.3 for what that leaves on the table), then multiplies the running object transform
//      in its registers: qvv_mul(local, object) and quat_normalize, the walk of kernels_consumers.inl per (child, parent) pair with the
//      same device functions.
//   5. the wave's 64 transforms leave through a 3 KiB LDS image as three 1 KiB streaming stores; a wave that withholds a request (a
//      refusal, the tail of the batch) stores per lane.
// Measured (MI355X, 65 536 characters of one 100-bone clip, tools/socket_requests.py, profiles/socket_requests.md) against object space
// poses into full rows + a gather: 1 socket 11.7 x (depth 3) / 5.1 x (depth 11), 4 sockets 9.3 x / 3.0 x, 16 sockets 3.2 x / 1.1 x;
// over 256 clips as drawn about half of each. Sixteen DEEP sockets per character do NOT beat the whole-pose route (0.78 x over 256
// clips): sockets that share a spine decode it once each, and step 4 is not packed across the wave.
// kMapped: skeleton space (chain over the skeleton's slots, local = the mapped track's decode or the reference pose).
// kMirrored: rtm::qvv_mul's matrix route is compiled in (launched while a registered clip or skeleton can hand out a negative scale);
// without it such a clip or skeleton -- registered behind a captured launch's back -- is refused, not computed wrongly.

	constexpr uint32_t k_bone_chain_levels = 16;
	constexpr uint32_t k_bone_stack_bytes = k_bone_chain_levels * k_wave_size * 2;			// [level][lane], 16 bits per transform
	constexpr uint32_t k_bone_lds_bytes_per_wave = k_track_image_bytes + k_bone_stack_bytes;	// image | stack; the record gather borrows the first 4 KiB
	static_assert(k_bone_lds_bytes_per_wave >= k_wave_size * k_clip_head_bytes && k_bone_lds_bytes_per_wave == k_track_lds_bytes_per_wave, "gather_clip_records stages 64 record heads in the wave's LDS");

	// what a lane keeps of its request's clip between levels (the seek's result and where the clip's tables are)
	struct bone_request_state
	{
		track_request_state seek;				// rows[] count back from the clip range table, as in decompress_track_requests
		const float4* base_pose;
		const clip_range_entry* clip_ranges;
		float lerp_alpha;
	};

	// The seek of one lane's request: everything decode_bone_local needs afterwards
	__device__ __forceinline__ void prepare_bone_request(const device_clip& clip, float sample_time, uint32_t rounding_policy, uint32_t looping_policy, bone_request_state& out)
	{
		seek_state state;
		seek(clip, sample_time, rounding_policy, looping_policy, state);
		out.seek.data[0] = state.animated_track_data[0];
		out.seek.data[1] = state.animated_track_data[1];
		out.seek.rows[0] = ((clip.num_segments - state.segment_index[0]) * clip.num_animated) | ((clip.flags & k_clip_short_exact_math) != 0 ? k_track_row_short_exact_math : 0u);
		out.seek.rows[1] = (clip.num_segments - state.segment_index[1]) * clip.num_animated;
		out.seek.bit_offsets[0] = state.key_frame_bit_offsets[0];
		out.seek.bit_offsets[1] = state.key_frame_bit_offsets[1];
		out.base_pose = clip.base_pose;
		out.clip_ranges = clip.clip_ranges;
		out.lerp_alpha = state.interpolation_alpha;
	}

	// The local transform of track `track` of the lane's clip at the request's sample time, as the pose consumers' images hold it: the
	// track_writer's own defaults, constants as stored, animated sub-tracks decoded (what launch_bone_requests restricts `params` to).
	// `active`: lanes that have a track to decode at this level (the others do nothing and return garbage).
	__device__ __forceinline__ qvv decode_bone_local(const bone_request_state& request, uint32_t track, bool active, uint32_t normalization)
	{
		float4 quads[3] = { make_float4(0.0f, 0.0f, 0.0f, 1.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(1.0f, 1.0f, 1.0f, 0.0f) };
		uint32_t animated = 0;
		if (active)
		{
			#pragma unroll
			for (uint32_t kind = 0; kind < 3; ++kind)
				quads[kind] = load_quad(request.base_pose, track * 3u + kind);
			#pragma unroll
			for (uint32_t kind = 0; kind < 3; ++kind)
			{
				const uint32_t marker = __float_as_uint(quads[kind].w);
				if (is_special_quad(marker))
				{
					if ((marker & k_quad_animated) != 0)
						animated |= 1u << kind;
					else
						quads[kind].w = (marker & k_quad_default_w_one) != 0 ? 1.0f : 0.0f;		// (the resolved pose's W of a default sub-track, host_clips.inl)
				}
			}
		}

		#pragma unroll 1
		for (uint32_t kind = 0; kind < 3; ++kind)
		{
			const bool decodes = ((animated >> kind) & 1u) != 0;
			if (__builtin_amdgcn_ballot_w64(decodes) == 0)
				continue;
			if (decodes)
			{
				const float4 tagged = kind == 0 ? quads[0] : (kind == 1 ? quads[1] : quads[2]);
				const uint32_t ordinal = __float_as_uint(tagged.w) & k_quad_ordinal_mask;
				// (plan_entry and clip_range_entry are both 32 bytes: the plan's last entry is clip_ranges[-1])
				const plan_entry* plan_end = reinterpret_cast<const plan_entry*>(request.clip_ranges);
				const uint32_t row0 = request.seek.rows[0] & ~k_track_row_short_exact_math, row1 = request.seek.rows[1];
				const plan_entry plan0 = load_entry(plan_end - row0, ordinal);
				const plan_entry plan1 = row1 == row0 ? plan0 : load_entry(plan_end - row1, ordinal);
				const clip_range_entry clip_range = load_entry(request.clip_ranges, ordinal);

				seek_state key_state;
				key_state.animated_track_data[0] = request.seek.data[0];
				key_state.animated_track_data[1] = request.seek.data[1];
				key_state.segment_index[0] = key_state.segment_index[1] = 0;		// (the rows are resolved already)
				key_state.key_frame_bit_offsets[0] = request.seek.bit_offsets[0];
				key_state.key_frame_bit_offsets[1] = request.seek.bit_offsets[1];
				key_state.interpolation_alpha = request.lerp_alpha;
				key_state.uses_single_segment = false;

				// the raw bit rate is rare: only a pass that actually meets one pays for its code path
				const bool has_raw = __any(int(is_raw_width(plan0.bit_offset_and_width >> 24) || is_raw_width(plan1.bit_offset_and_width >> 24))) != 0;
				const bool short_exact_math = (request.seek.rows[0] & k_track_row_short_exact_math) != 0;
				float4 value;
				if (!has_raw)
					value = decode_animated_sub_track<false, false, k_track_wide_key_loads>(key_state, plan0, plan1, clip_range, kind == 0, k_round_none, request.lerp_alpha, normalization, false, short_exact_math);
				else
					value = decode_animated_sub_track<true, false, k_track_wide_key_loads>(key_state, plan0, plan1, clip_range, kind == 0, k_round_none, request.lerp_alpha, normalization, false, false);
				if (kind == 0)
					quads[0] = value;
				else if (kind == 1)
					quads[1] = value;
				else
					quads[2] = value;
			}
		}

		qvv local;
		local.rotation = quads[0];
		local.translation = make_float4(quads[1].x, quads[1].y, quads[1].z, 0.0f);
		local.scale = make_float4(quads[2].x, quads[2].y, quads[2].z, 0.0f);
		return local;
	}

	template<bool kMapped, bool kMirrored>
	__global__ __launch_bounds__(k_block_size) void decompress_bone_object_kernel(const device_clip* __restrict__ clips, uint32_t num_clips,
		const uint32_t* __restrict__ clip_ids, const float* __restrict__ sample_times, const uint32_t* __restrict__ bones, uint32_t num_requests,
		decode_params params, float4* __restrict__ transforms, unsigned long long* __restrict__ rejected_count, skeleton_launch mapping)
	{
		__shared__ __attribute__((aligned(16))) uint8_t bone_lds[k_waves_per_block * k_bone_lds_bytes_per_wave];

		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		const uint32_t first_request = (blockIdx.x * k_waves_per_block + wave_in_block) * k_wave_size;		// wave uniform
		if (first_request >= num_requests)
			return;
		const uint32_t request_index = first_request + lane;
		const bool in_batch = request_index < num_requests;

		uint8_t* wave_lds = bone_lds + wave_in_block * k_bone_lds_bytes_per_wave;
		f32x4* image = reinterpret_cast<f32x4*>(wave_lds);													// [request * 3 + kind]
		uint16_t* stack = reinterpret_cast<uint16_t*>(wave_lds + k_track_image_bytes) + lane;				// [level * 64]: the lane's own column

		// ---- 1. lanes <-> requests ---------------------------------------------------------------------------------------------------
		const uint32_t clamped_request = in_batch ? request_index : first_request;
		const uint32_t clip_id = clip_ids[clamped_request];
		const float sample_time = sample_times[clamped_request];
		const uint32_t bone = bones[clamped_request];
		const uint32_t rounding_policy = instance_rounding_policy_of(params, clamped_request);
		const uint32_t looping_policy = instance_looping_policy_of(params, clamped_request);

		const bool known_clip = in_batch && clip_id < num_clips;
		const uint32_t first_clip_id = __builtin_amdgcn_readfirstlane(clip_id);			// lane 0 is always in the batch
		const bool shared_clip = __builtin_amdgcn_ballot_w64(in_batch && clip_id != first_clip_id) == 0 && first_clip_id < num_clips;	// wave uniform

		// skeleton space: the request's skeleton and its clip's map. A cleared record (an unknown or retired handle) holds no image;
		// record 0 of both tables is never handed out.
		const uint32_t* hierarchy = nullptr;
		uint32_t num_bones = 0;
		const f32x4* reference_pose = nullptr;
		const ACLHIP_CONSTANT uint32_t* slot_to_track = nullptr;
		bool mapping_fits = true;
		uint32_t map_tracks = 0;
		uint32_t short_exact = 1;
		bool negative_scale = false;
		if constexpr (kMapped)
		{
			const uint32_t skeleton_id = mapping.instance_skeletons != nullptr ? mapping.instance_skeletons[clamped_request] : mapping.skeleton;
			const uint32_t map_id = mapping.instance_maps != nullptr ? mapping.instance_maps[clamped_request] : mapping.map;
			const device_skeleton skeleton = load_entry(mapping.skeletons, skeleton_id < mapping.num_skeletons ? skeleton_id : 0);
			const device_track_map map = load_entry(mapping.maps, map_id < mapping.num_maps ? map_id : 0);
			mapping_fits = skeleton_id < mapping.num_skeletons && skeleton.reference_pose != nullptr
				&& map_id < mapping.num_maps && map.image != nullptr && map.num_slots == skeleton.num_bones;
			hierarchy = skeleton.hierarchy;
			num_bones = skeleton.num_bones;
			reference_pose = skeleton.reference_pose;
			slot_to_track = slot_to_track_of(map);
			map_tracks = map.num_tracks;
			short_exact = (skeleton.flags & k_skeleton_short_exact_math) != 0 ? 1u : 0u;		// (the reference pose fills slots: its rotations are multiplied too)
			negative_scale = (skeleton.flags & k_skeleton_negative_scale) != 0;
		}

		// refused: unknown / scalar clips, a clip (a skeleton) without hierarchy, a bone the pose does not have, unknown or retired
		// skeletons and maps, a map made for another clip or another skeleton, and -- launches compiled without the matrix route -- a clip
		// or a skeleton that may hand out a negative scale
		const auto accepts = [&](const device_clip& clip)
		{
			bool accepted = is_transform_clip(clip.flags) && (kMirrored || (!negative_scale && (clip.flags & k_clip_negative_scale) == 0));
			if constexpr (kMapped)
				accepted = accepted && mapping_fits && map_tracks == clip.num_tracks;
			else
			{
				hierarchy = clip.hierarchy;
				num_bones = clip.num_tracks;
			}
			short_exact &= walk_may_use_short_exact_math(clip.flags, params.normalization);
			return accepted && hierarchy != nullptr && bone < num_bones;
		};

		bone_request_state request = {};
		bool accepted = false;
		if (shared_clip)
		{
			const device_clip clip = load_clip(clips, first_clip_id);
			accepted = in_batch && accepts(clip);
			if (accepted)
				prepare_bone_request(clip, sample_time, rounding_policy, looping_policy, request);
		}
		else
		{
			const device_clip clip = gather_clip_records(clips, num_clips, clip_id, known_clip, lane, wave_lds, true);
			accepted = known_clip && accepts(clip);
			if (accepted)
				prepare_bone_request(clip, sample_time, rounding_policy, looping_policy, request);
		}

		// refused requests are counted, one atomic per wave
		const uint64_t refused = __builtin_amdgcn_ballot_w64(in_batch && !accepted);
		if (refused != 0 && lane == 0)
			atomicAdd(rejected_count, (unsigned long long)__builtin_popcountll(refused));

		// ---- 2. the chain, root first ----------------------------------------------------------------------------------------------------
		// the hierarchy's parent table: its offset is the fourth word of the image's first header (build_walk_schedule_image)
		const ACLHIP_CONSTANT uint32_t* parents = nullptr;
		uint32_t depth = 0;				// ancestors of the bone
		if (accepted)
		{
			parents = as_constant(hierarchy) + as_constant(hierarchy)[3];
			depth = parents[bone] >> 16;
		}
		// the short exact normalize for the whole wave or not at all (the same bits either way: DESIGN.md 4.1)
		const bool short_exact_wave = __builtin_amdgcn_ballot_w64(accepted && short_exact == 0) == 0;

		qvv object;
		object.rotation = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
		object.translation = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		object.scale = make_float4(1.0f, 1.0f, 1.0f, 0.0f);

		#pragma unroll 1
		for (uint32_t segment = 0; __builtin_amdgcn_ballot_w64(accepted && segment <= depth) != 0; segment += k_bone_chain_levels)
		{
			// climb from the bone to the segment's first level; the transforms of levels [segment, segment + 16) go on the stack
			if (accepted && segment <= depth)
			{
				uint32_t transform = bone;
				for (uint32_t level = depth; ; --level)
				{
					if (level - segment < k_bone_chain_levels)
						stack[(level - segment) * k_wave_size] = uint16_t(transform);
					if (level == segment)
						break;
					transform = parents[transform] & 0xFFFFu;
				}
			}

			#pragma unroll 1
			for (uint32_t step = 0; step < k_bone_chain_levels; ++step)
			{
				const uint32_t level = segment + step;
				const bool active = accepted && level <= depth;
				if (__builtin_amdgcn_ballot_w64(active) == 0)
					break;
				const uint32_t transform = active ? uint32_t(stack[step * k_wave_size]) : 0u;

				qvv local;
				if constexpr (kMapped)
				{
					// the slot's track through the map, or the reference pose where no track maps to the slot
					const uint32_t track = active ? slot_to_track[transform] : ACLHIP_TRACK_DROPPED;
					local = decode_bone_local(request, track, active && track != ACLHIP_TRACK_DROPPED, params.normalization);
					if (active && track == ACLHIP_TRACK_DROPPED)
						local = load_qvv(reference_pose, transform);
				}
				else
					local = decode_bone_local(request, transform, active, params.normalization);

				if (active && level == 0)
					object = local;			// a root: as decoded, nothing applied to it
				else if (active)
				{
					// the walk of kernels_consumers.inl for one (child, parent) pair
					qvv product = qvv_mul(local, object);
					if constexpr (kMirrored)
					{
						const bool mirrored = qvv_mul_takes_matrix_path(local, object);
						if (__builtin_amdgcn_ballot_w64(mirrored) != 0 && mirrored)
							product = qvv_mul_through_matrices(local, object);
					}
					if (short_exact_wave)		// (a scalar branch)
						product.rotation = quat_normalize<true>(product.rotation);
					else
						product.rotation = quat_normalize<false>(product.rotation);
					object = product;
				}
			}
		}

		// ---- 3. the wave's 64 transforms leave -----------------------------------------------------------------------------------------
		if (__builtin_amdgcn_ballot_w64(accepted) == ~0ull)
		{
			// three 1 KiB contiguous stores
			store_qvv(image, lane, object);
			track_wave_barrier();
			f32x4 staged[3];
			#pragma unroll
			for (uint32_t row = 0; row < 3; ++row)
				staged[row] = image[row * k_wave_size + lane];
			float4* out = transforms + size_t(first_request) * 3u + lane;
			#pragma unroll
			for (uint32_t row = 0; row < 3; ++row)
				store_streaming(out + row * k_wave_size, staged[row]);
			return;
		}

		// a refused request leaves its 48 bytes as the caller had them
		if (accepted)
		{
			float4* out = transforms + size_t(request_index) * 3u;
			store_streaming(out + 0, f32x4{ object.rotation.x, object.rotation.y, object.rotation.z, object.rotation.w });
			store_streaming(out + 1, f32x4{ object.translation.x, object.translation.y, object.translation.z, 0.0f });
			store_streaming(out + 2, f32x4{ object.scale.x, object.scale.y, object.scale.z, 0.0f });
		}
	}
