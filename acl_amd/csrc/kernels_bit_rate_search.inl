// kernels_bit_rate_search.inl -- part of aclhip.hip (one translation unit; included there behind kernels_variable_compress.inl, not compiled on its own).
// aclhip_find_bit_rates_batch: the reference's find_optimal_bit_rates (compression/impl/quantize.transform.h:1174-1523) at the levels
// lowest, low and medium for quatf_drop_w_variable / vector3f_variable / vector3f_variable: the rate table
// aclhip_compress_tracks_variable_batch reads. The error metric (aclhip_find_bit_rates_metric_batch) is a template argument of the local
// and of the object kernel, as of the two launches in front of them: the qvvf instantiations are the kernels without it, the matrix
// ones take S2 with scale through matrix_from_qvv, matrix_mul and matrix_shell_error (kernels_pose_buffers.inl). Five stream ordered launches:
//   tracks_compress_shell_kernel         (kernels_tracks_compress.inl, unchanged) the refusals, the finite test, the clip's rigid shell, the vote
//   variable_compress_analyze_kernel     (kernels_variable_compress.inl, unchanged) the sub-track types and the clip ranges
//   bit_rate_search_segment_kernel       per (instance, segment): the segment ranges as six floats per animated sub-track (lanes <->
//                                        sub-tracks), then the SEGMENT'S shell from what its streams hold (tracks descending, samples
//                                        across the lanes); the segment's record; segment 0 takes the instance's result
//   bit_rate_search_local_kernel         per (instance, segment, track): an LDS table of the value every rate stands for at every sample,
//                                        then the permutation list one size class at a time, lanes <-> permutations, each lane scanning
//                                        the samples until its error is too high; (smallest error, first index) by butterfly
//   bit_rate_search_object_kernel        per (instance, segment): the tracks parent first, lanes <-> samples, the chain walked per lane
//                                        from the root for every candidate; every decision wave uniform behind a reduction
// include/aclhip.h states the definition (S0 to S4): fp32, one IEEE operation at a time. No atomics besides the refusal counter and no
// zero fill: the same bytes on every run. The rates live in the caller's table between the last two launches and while the object
// phase works: every lane stores the same four bytes and reads back what it stored itself.
// aclhip_find_bit_rates_level_batch (the levels high and highest, and automatic) is these with one small launch in front of the
// object phase, bit_rate_search_level_kernel (the level per instance), and the object kernel's second instantiation, kLevels: its
// first loop tries the wider shapes of increments over the chain. The kernels of the other two calls are the instantiations without.
// aclhip_find_bit_rates_additive_batch is that call with the kAdditive instantiations of the segment kernel (S0), the local and the
// object kernel, as of the two launches in front of them: every transform S0 and S2 look at goes through A on the instance's base
// (kernels_tracks_compress.inl: compress_additive_base) first.

	constexpr uint32_t k_search_num_rates = 25;					// 0 .. 24
	constexpr uint32_t k_search_invalid_rates = 0x00FFFFFFu;		// { 255, 255, 255, 0 }: no sub-track of the track is animated
	constexpr uint32_t k_search_memo_unset = 0xFFFFFFFFu;		// (no packed rates: their fourth byte is 0)
	constexpr uint32_t k_search_segment_floats = 18;			// per track: pmin xyz, pext xyz of the rotation, the translation, the scale

	// ---- the permutation lists ---------------------------------------------------------------------------------------------------------------
	// The reference's lists of 1, 2 and 3 rates (transform_bit_rate_permutations.h) are made by a script from one rule: every tuple of
	// rates 0 .. 24, sorted by the bits of the transform -- the sum over its kinds of the bits of a component, 32 at rate 24 --, then by the
	// rates themselves, the first kind first. Made here at compile time from that rule by a counting sort over the tuples in ascending
	// order (stable: ties keep the order of the rates). An entry is rate 0 | rate 1 << 8 | rate 2 << 16 | the summed bits << 24.
	constexpr uint32_t search_rate_bits(uint32_t rate) { return rate == k_variable_raw_rate ? 32u : rate; }
	template<uint32_t kCount> struct search_permutation_list { uint32_t entries[kCount]; };
	template<uint32_t kKinds, uint32_t kCount>
	constexpr search_permutation_list<kCount> make_search_permutations()
	{
		search_permutation_list<kCount> list = {};
		uint32_t at[98] = {};
		for (uint32_t a = 0; a < k_search_num_rates; ++a)
			for (uint32_t b = 0; b < (kKinds > 1 ? k_search_num_rates : 1u); ++b)
				for (uint32_t c = 0; c < (kKinds > 2 ? k_search_num_rates : 1u); ++c)
					++at[search_rate_bits(a) + (kKinds > 1 ? search_rate_bits(b) : 0u) + (kKinds > 2 ? search_rate_bits(c) : 0u) + 1u];
		for (uint32_t size = 1; size < 98; ++size)
			at[size] += at[size - 1];
		for (uint32_t a = 0; a < k_search_num_rates; ++a)
			for (uint32_t b = 0; b < (kKinds > 1 ? k_search_num_rates : 1u); ++b)
				for (uint32_t c = 0; c < (kKinds > 2 ? k_search_num_rates : 1u); ++c)
				{
					const uint32_t size = search_rate_bits(a) + (kKinds > 1 ? search_rate_bits(b) : 0u) + (kKinds > 2 ? search_rate_bits(c) : 0u);
					list.entries[at[size]++] = a | (b << 8) | (c << 16) | (size << 24);
				}
		return list;
	}
	__device__ const search_permutation_list<25> k_search_permutations_1 = make_search_permutations<1, 25>();
	__device__ const search_permutation_list<625> k_search_permutations_2 = make_search_permutations<2, 625>();
	__device__ const search_permutation_list<15625> k_search_permutations_3 = make_search_permutations<3, 15625>();

	// What the segment launch leaves of a (instance, segment) for the two behind it
	struct search_segment
	{
		uint32_t start, count;					// the segment's samples
		uint32_t has_scale;						// not every scale of the instance is default
		uint32_t valid;							// 0: the instance ended with a status or has no such segment: nothing is searched, no row is written
	};
	static_assert(sizeof(search_segment) == 16, "one dwordx4 load");

	struct bit_rate_search_launch
	{
		variable_compress_launch variable;		// what the shell and the analysis read and leave
		uint8_t* table;							// { rotation, translation, scale, 0 } per (instance, segment, track)
		uint64_t instance_stride, segment_stride;
		search_segment* segments;				// [num_instances][max_segments]
		float* segment_ranges;					// [num_instances][max_segments][max_tracks][18]
		float2* segment_shells;					// [num_instances][max_segments][max_tracks] { local shell distance, precision } of S0
		uint16_t* chains;						// [num_instances][max_segments][max_tracks]: the chain of the track under work, from the root
	};

	// and what aclhip_find_bit_rates_level_batch has besides: a record of its own, for its two kernels alone (the kernel arguments of
	// the others stay as they are)
	struct bit_rate_search_levels_launch
	{
		bit_rate_search_launch search;
		uint32_t* memo;							// [num_instances][max_segments][max_tracks][3]: per link of the chain under work, increase_bone_bit_rate by 1, 2 and 3 of this round
		uint32_t level;							// an acl::compression_level8: 0 .. 4, or ACLHIP_LEVEL_AUTOMATIC
	};
	__device__ __forceinline__ const bit_rate_search_launch& search_launch_of(const bit_rate_search_launch& launch) { return launch; }
	__device__ __forceinline__ const bit_rate_search_launch& search_launch_of(const bit_rate_search_levels_launch& launch) { return launch.search; }

	// What S0 and S1 read of an (instance, segment)
	struct search_source
	{
		const f32x4* samples;
		size_t pose_quads;
		const float* clip_ranges;				// the instance's
		const float* segment_ranges;			// the segment's
		const f32x4* default_pose;
		uint32_t start, count;
		bool multiple;
	};

	__device__ __forceinline__ float4 search_normalize(float4 q)
	{
		const float inv_length = 1.0f / sqrtf((q.x * q.x + q.z * q.z) + (q.y * q.y + q.w * q.w));
		return make_float4(q.x * inv_length, q.y * inv_length, q.z * inv_length, q.w * inv_length);
	}

	// rotation_to_quat_32 of a drop-w rotation, then rtm::quat_normalize
	__device__ __forceinline__ float4 search_rotation_of(float3 v) { return search_normalize(make_float4(v.x, v.y, v.z, quat_from_positive_w(v.x, v.y, v.z))); }

	// the raw local transform of the metric: the registered sample with its rotation normalized (tracks_compress_sample does that: step 1,
	// clip_context.impl.h:150), of positive w, and normalized a second time here (sample_streams.h:611-625 normalizes what it reads)
	__device__ __forceinline__ qvv search_raw_local(const search_source& source, uint32_t track, uint32_t sample)
	{
		qvv raw = tracks_compress_sample(source.samples, source.pose_quads, sample, track);
		raw.rotation = search_normalize(tracks_compress_positive_w(raw.rotation));
		return raw;
	}

	__device__ __forceinline__ float3 search_default_value(const search_source& source, uint32_t track, uint32_t kind)
	{
		if (source.default_pose == nullptr)
			return kind == 2 ? make_float3(1.0f, 1.0f, 1.0f) : make_float3(0.0f, 0.0f, 0.0f);
		const f32x4 v = source.default_pose[size_t(track) * 3u + kind];
		return make_float3(v.x, v.y, v.z);
	}

	// the doubly (with one segment: singly) normalized sample a segment's stream holds of an animated sub-track
	__device__ __forceinline__ float3 search_normalized(const search_source& source, uint32_t track, uint32_t kind, uint32_t sample)
	{
		float3 v = variable_compress_normalize3(variable_compress_value(source.samples, source.pose_quads, sample, track, kind), source.clip_ranges + size_t(track) * k_variable_range_floats + kind * 6u);
		if (source.multiple)
			v = variable_compress_normalize3(v, source.segment_ranges + size_t(track) * k_search_segment_floats + kind * 6u);
		return v;
	}

	__device__ __forceinline__ float search_decay(float value, uint32_t bits)
	{
		const float most = float((1u << bits) - 1u);
		return floorf(value * most + 0.5f) * (1.0f / most);
	}

	// S1: x, y, z an animated sub-track gives at `rate` for sample `sample` of the clip (sample_streams.h:163-212, 306-355)
	__device__ __forceinline__ float3 search_value(const search_source& source, uint32_t track, uint32_t kind, uint32_t rate, uint32_t sample)
	{
		if (rate >= k_variable_raw_rate)
			return variable_compress_value(source.samples, source.pose_quads, sample, track, kind);
		const float* clip_range = source.clip_ranges + size_t(track) * k_variable_range_floats + kind * 6u;
		float3 v;
		if (rate == 0)
		{
			v = variable_compress_normalize3(variable_compress_value(source.samples, source.pose_quads, source.start, track, kind), clip_range);
			v = make_float3(search_decay(v.x, 16), search_decay(v.y, 16), search_decay(v.z, 16));
		}
		else
		{
			v = search_normalized(source, track, kind, sample);
			v = make_float3(search_decay(v.x, rate), search_decay(v.y, rate), search_decay(v.z, rate));
			if (source.multiple)
			{
				const float* range = source.segment_ranges + size_t(track) * k_search_segment_floats + kind * 6u;
				v = make_float3(v.x * range[3] + range[0], v.y * range[4] + range[1], v.z * range[5] + range[2]);
			}
		}
		return make_float3(v.x * clip_range[3] + clip_range[0], v.y * clip_range[4] + clip_range[1], v.z * clip_range[5] + clip_range[2]);
	}

	// what a sub-track that is not animated contributes: sample 0 of a constant one (the rotation normalized a second time: search_raw_local), the default as given
	__device__ __forceinline__ float4 search_fixed_value(const search_source& source, uint32_t track, uint32_t kind, uint32_t type)
	{
		if (type == k_sub_track_default)
		{
			if (source.default_pose == nullptr)
				return kind == 0 ? make_float4(0.0f, 0.0f, 0.0f, 1.0f) : kind == 1 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(1.0f, 1.0f, 1.0f, 0.0f);
			const f32x4 v = source.default_pose[size_t(track) * 3u + kind];
			return make_float4(v.x, v.y, v.z, kind == 0 ? v.w : 0.0f);
		}
		const qvv first = search_raw_local(source, track, 0);
		return kind == 0 ? first.rotation : kind == 1 ? first.translation : first.scale;
	}

	// the S1 transform of a track at its three rates (packed: rotation | translation << 8 | scale << 16) for a sample of the segment
	__device__ __forceinline__ qvv search_lossy_local(const search_source& source, uint32_t track, uint32_t flags, uint32_t rates, uint32_t sample_in_segment)
	{
		float4 parts[3];
		#pragma unroll
		for (uint32_t kind = 0; kind < 3; ++kind)
		{
			const uint32_t type = (flags >> (2u * kind)) & 3u;
			if (type == k_sub_track_animated)
			{
				const float3 v = search_value(source, track, kind, (rates >> (8u * kind)) & 0xFFu, source.start + sample_in_segment);
				parts[kind] = kind == 0 ? search_rotation_of(v) : make_float4(v.x, v.y, v.z, 0.0f);
			}
			else
				parts[kind] = search_fixed_value(source, track, kind, type);
		}
		qvv lossy;
		lossy.rotation = parts[0];
		lossy.translation = parts[1];
		lossy.scale = parts[2];
		return lossy;
	}

	// S2: calculate_error of the metric, or calculate_error_no_scale: the x and the y point only, no scale (transform_error_metrics.h:335-378;
	// the matrix metric inherits it: without scale both metrics are one)
	template<uint32_t kMetric>
	__device__ __forceinline__ float search_error(bool has_scale, float distance, const qvv& raw, const qvv& lossy)
	{
		if (has_scale)
			return compress_shell_error<kMetric>(distance, raw, lossy);
		qvv raw_rigid = raw, lossy_rigid = lossy;
		raw_rigid.scale = lossy_rigid.scale = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
		const float error_x = shell_point_error(distance, 0.0f, 0.0f, raw_rigid, lossy_rigid);
		const float error_y = shell_point_error(0.0f, distance, 0.0f, raw_rigid, lossy_rigid);
		return error_x > error_y ? error_x : error_y;
	}

	// qvv_normalize(qvv_mul(local, parent)), or its _no_scale twin (transform_error_metrics.h:289-333); the quaternion path
	__device__ __forceinline__ qvv search_to_object(bool has_scale, const qvv& local, const qvv& parent)
	{
		qvv over = parent;
		if (!has_scale)
			over.scale = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
		qvv result;
		result.rotation = search_normalize(quat_mul(local.rotation, parent.rotation));
		result.translation = qvv_mul_point3(local.translation.x, local.translation.y, local.translation.z, over);
		result.scale = has_scale ? make_float4(local.scale.x * parent.scale.x, local.scale.y * parent.scale.y, local.scale.z * parent.scale.z, 0.0f) : over.scale;
		return result;
	}

	// S2's base sample (kAdditive): what sample_streams gives of the base (sample_streams.h:649-673) -- base(b, s) at the same nearest
	// key, its rotation normalized ONCE MORE, a quat_normalize of the already normalized value, as written there
	__device__ __forceinline__ qvv search_base_local(const compress_additive_base& base, uint32_t track, uint32_t key)
	{
		qvv transform = compress_base_sample(base, track, key);
		transform.rotation = search_normalize(transform.rotation);
		return transform;
	}

	// S2's A: apply_additive_to_base, or without has_scale apply_additive_to_base_no_scale (core/additive_utils.h:145-174): relative is
	// rtm::qvv_mul_no_scale(additive, base), additive0 and additive1 are transform_add_no_scale; the scale is 1
	__device__ __forceinline__ qvv search_apply_additive(bool has_scale, const compress_additive_base& base, const qvv& base_transform, const qvv& additive)
	{
		if (has_scale)
			return compress_apply_additive(base, base_transform, additive);
		qvv result;
		result.rotation = quat_mul(additive.rotation, base_transform.rotation);
		const float4 moved = base.format == 1 ? quat_mul_vector3(additive.translation, base_transform.rotation) : additive.translation;
		result.translation = make_float4(moved.x + base_transform.translation.x, moved.y + base_transform.translation.y, moved.z + base_transform.translation.z, 0.0f);
		result.scale = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
		return result;
	}

	// ---- per (instance, segment): the segment ranges, the segment's shell, the record ------------------------------------------------------------
	// kAdditive: S0's stretch over A(what the segment's streams hold) with base(b, s), s the index in the clip (rigid_shell_utils.h:220-242)
	template<bool kAdditive = false>
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void bit_rate_search_segment_kernel(bit_rate_search_launch launch)
	{
		const transform_compress_launch& base = launch.variable.base;
		const uint32_t max_segments = launch.variable.max_segments;
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint64_t num_waves = uint64_t(base.num_instances) * max_segments;
		for (uint64_t wave = uint64_t(blockIdx.x) * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size); wave < num_waves;
			wave += uint64_t(gridDim.x) * k_compress_waves_per_block)
		{
			const uint32_t instance = uint32_t(wave / max_segments), segment = uint32_t(wave % max_segments);
			const compress_instance voted = load_compress_instance(base.instances, instance);
			uint32_t status = voted.status;
			if (status == 0 && voted.num_out_samples > launch.variable.max_samples)
				status = k_compress_status_refused;
			if (segment == 0 && lane == 0)
			{
				const uint32_t result = status == 0 ? ACLHIP_COMPRESS_OK : (status & k_compress_status_refused) != 0 ? ACLHIP_COMPRESS_REFUSED : ACLHIP_COMPRESS_NOT_FINITE;
				base.results[instance] = make_uint2(result, 0);
				if (result == ACLHIP_COMPRESS_REFUSED)
					atomicAdd(base.rejected_count, 1ull);
			}
			const variable_split split = variable_split_of(voted.num_out_samples);
			search_segment out = { 0, 0, 0, 0 };
			if (status != 0 || segment >= split.num_segments || voted.num_out_samples == 0)
			{
				if (lane == 0)
					launch.segments[wave] = out;
				continue;
			}
			variable_segment_samples(split, segment, out.start, out.count);
			const uint32_t handle = as_constant(base.raws)[instance];
			const device_raw_tracks raw = load_raw_tracks_fields(base.arrays, handle < base.num_arrays ? handle : 0);
			const uint32_t num_tracks = voted.num_tracks;
			const uint8_t* track_flags = base.track_flags + size_t(instance) * base.max_tracks;

			search_source source;
			source.samples = raw.samples;
			source.pose_quads = size_t(num_tracks) * 3u;
			source.clip_ranges = launch.variable.clip_ranges + size_t(instance) * base.max_tracks * k_variable_range_floats;
			source.segment_ranges = launch.segment_ranges + wave * base.max_tracks * k_search_segment_floats;
			source.default_pose = base.default_pose;
			source.start = out.start;
			source.count = out.count;
			source.multiple = split.num_segments > 1;

			// the ranges: a lane per sub-track; has_scale: not every scale is default
			float* ranges = launch.segment_ranges + wave * base.max_tracks * k_search_segment_floats;
			bool scaled = false;
			for (uint32_t index = lane; index < num_tracks * 3u; index += k_wave_size)
			{
				const uint32_t track = index / 3u, kind = index - track * 3u;
				const uint32_t type = (track_flags[track] >> (2u * kind)) & 3u;
				scaled = scaled || (kind == 2 && type != k_sub_track_default);
				if (type != k_sub_track_animated || !source.multiple)
					continue;
				const float* clip_range = source.clip_ranges + size_t(track) * k_variable_range_floats + kind * 6u;
				float2 padded[3];
				variable_segment_range(source.samples, source.pose_quads, track, kind, clip_range, out.start, out.count, padded);
				#pragma unroll
				for (uint32_t c = 0; c < 3; ++c)
				{
					ranges[size_t(track) * k_search_segment_floats + kind * 6u + c] = padded[c].x;
					ranges[size_t(track) * k_search_segment_floats + kind * 6u + 3u + c] = padded[c].y;
				}
			}
			out.has_scale = __ballot(scaled) != 0 ? 1u : 0u;
			out.valid = 1;
			if (lane == 0)
				launch.segments[wave] = out;
			__threadfence();		// (the ranges are read back below by other lanes of this wave)

			// S0: the segment's shell, tracks_compress_shell_kernel's walk over what the segment's streams hold (spelled out here, the
			// settings included: with any of it shared this kernel takes 65 VGPRs where it takes 61, a wave a SIMD less)
			float2* shells = launch.segment_shells + wave * base.max_tracks;
			for (uint32_t track = lane; track < num_tracks; track += k_wave_size)
				shells[track] = make_float2(base.track_shell_distances != nullptr ? base.track_shell_distances[track] : base.shell_distance,
					base.track_precisions != nullptr ? base.track_precisions[track] : base.precision);
			__threadfence();		// (a lane's entry is read below by every lane)
			const uint32_t sample = lane < out.count ? lane : 0u;
			[[maybe_unused]] compress_additive_base additive = {};
			[[maybe_unused]] uint32_t base_key = 0;
			if constexpr (kAdditive)
			{
				additive = compress_additive_base_of(base, instance, raw);
				base_key = compress_base_key(additive, out.start + sample);
			}
			for (uint32_t track = num_tracks; track-- != 0;)
			{
				const float2 shell = shells[track];
				const float distance = shell.x;
				const uint32_t flags = track_flags[track];
				float3 stored[3];
				#pragma unroll
				for (uint32_t kind = 0; kind < 3; ++kind)
				{
					const uint32_t type = (flags >> (2u * kind)) & 3u;
					if (type == k_sub_track_animated)
						stored[kind] = search_normalized(source, track, kind, out.start + sample);
					else if (type == k_sub_track_constant)
						stored[kind] = variable_compress_value(source.samples, source.pose_quads, 0, track, kind);
					else
						stored[kind] = search_default_value(source, track, kind);
				}
				qvv transform;
				transform.rotation = search_rotation_of(stored[0]);
				transform.translation = make_float4(stored[1].x, stored[1].y, stored[1].z, 0.0f);
				transform.scale = make_float4(stored[2].x, stored[2].y, stored[2].z, 0.0f);
				if constexpr (kAdditive)
					transform = compress_apply_additive(additive, compress_base_sample(additive, track, base_key), transform);
				float stretch = 0.0f;
				if (lane < out.count)
				{
					const float length_x = tracks_compress_length3(qvv_mul_point3(distance, 0.0f, 0.0f, transform));
					const float length_y = tracks_compress_length3(qvv_mul_point3(0.0f, distance, 0.0f, transform));
					const float length_z = tracks_compress_length3(qvv_mul_point3(0.0f, 0.0f, distance, transform));
					stretch = length_x > stretch ? length_x : stretch;
					stretch = length_y > stretch ? length_y : stretch;
					stretch = length_z > stretch ? length_z : stretch;
				}
				stretch = compress_wave_max(stretch);
				const float own_distance = base.track_shell_distances != nullptr ? base.track_shell_distances[track] : base.shell_distance;
				const float own_precision = base.track_precisions != nullptr ? base.track_precisions[track] : base.precision;
				const float parent_shell_distance = distance != own_distance ? stretch + own_precision : stretch;
				const uint32_t parent = base.parent_indices != nullptr ? base.parent_indices[track] : ACLHIP_NO_PARENT;
				if (parent < track && parent_shell_distance > shells[parent].x)
					shells[parent] = make_float2(parent_shell_distance, shell.y);
			}
		}
	}

	// ---- per (instance, segment, track): the local phase -----------------------------------------------------------------------------------------
	// S3. One wave64 a block. The table: for every animated kind of the track, every rate and every sample of the segment the S1 value (a
	// rotation with its w, normalized), 31 KiB of LDS; the raw local transforms beside it. Then the track's permutation list in order, one
	// size class at a time -- a round takes the lanes that share the size of the first entry not yet tried --: a lane scans the samples
	// until its error is >= the threshold and keeps the maximum so far; the wave keeps the smallest error and, of equals, the first
	// entry: what the reference's sequence of strict `<` updates keeps. A class that ends good enough ends the list.
	// kAdditive: the raw table holds A(raw), and every candidate's S1 transform goes through A at its sample. The segment's base samples
	// (search_base_local) stay in registers, lane l holding sample l's: the scan's sample is the same in every lane that still scans, so
	// ten v_readlane fetch it. (In LDS beside the raw table they cost 1 240 bytes, and the fifth block of a CU with them.)
	template<uint32_t kMetric, bool kAdditive = false>
	__global__ __launch_bounds__(k_wave_size) void bit_rate_search_local_kernel(bit_rate_search_launch launch)
	{
		__shared__ float4 rotation_table[k_search_num_rates * k_variable_max_samples];
		__shared__ float vector_table[2][k_search_num_rates * k_variable_max_samples * 3u];
		__shared__ float raw_table[k_variable_max_samples * 10u];

		const transform_compress_launch& base = launch.variable.base;
		const uint32_t max_segments = launch.variable.max_segments;
		const uint32_t lane = threadIdx.x;
		const uint64_t num_waves = uint64_t(base.num_instances) * max_segments * base.max_tracks;
		for (uint64_t wave = blockIdx.x; wave < num_waves; wave += gridDim.x)
		{
			const uint32_t track = uint32_t(wave % base.max_tracks);
			const uint64_t segment_index = wave / base.max_tracks;
			const uint32_t instance = uint32_t(segment_index / max_segments), segment = uint32_t(segment_index % max_segments);
			const search_segment at = launch.segments[segment_index];
			if (at.valid == 0)
				continue;
			const compress_instance voted = load_compress_instance(base.instances, instance);
			if (track >= voted.num_tracks)
				continue;
			const uint32_t handle = as_constant(base.raws)[instance];
			const device_raw_tracks raw = load_raw_tracks_fields(base.arrays, handle < base.num_arrays ? handle : 0);
			const uint32_t flags = base.track_flags[size_t(instance) * base.max_tracks + track];
			uint32_t* row = reinterpret_cast<uint32_t*>(launch.table + instance * launch.instance_stride + segment * launch.segment_stride) + track;

			// the k-th animated kind (every index a constant: no scratch)
			const bool animated_rotation = (flags & 3u) == k_sub_track_animated, animated_translation = ((flags >> 2) & 3u) == k_sub_track_animated;
			const uint32_t num_kinds = (animated_rotation ? 1u : 0u) + (animated_translation ? 1u : 0u) + (((flags >> 4) & 3u) == k_sub_track_animated ? 1u : 0u);
			const uint32_t kinds[3] = { animated_rotation ? 0u : animated_translation ? 1u : 2u, animated_rotation && animated_translation ? 1u : 2u, 2u };
			if (num_kinds == 0)
			{
				if (lane == 0)
					*row = k_search_invalid_rates;
				continue;
			}

			search_source source;
			source.samples = raw.samples;
			source.pose_quads = size_t(voted.num_tracks) * 3u;
			source.clip_ranges = launch.variable.clip_ranges + size_t(instance) * base.max_tracks * k_variable_range_floats;
			source.segment_ranges = launch.segment_ranges + segment_index * base.max_tracks * k_search_segment_floats;
			source.default_pose = base.default_pose;
			source.start = at.start;
			source.count = at.count;
			source.multiple = variable_split_of(voted.num_out_samples).num_segments > 1;
			const bool has_scale = at.has_scale != 0;
			const float2 shell = launch.segment_shells[segment_index * base.max_tracks + track];

			__syncthreads();		// (the round before this one has read its tables)
			for (uint32_t index = lane; index < k_search_num_rates * at.count; index += k_wave_size)
			{
				const uint32_t rate = index / at.count, sample = index - rate * at.count;
				if (rate == 0 && !source.multiple)
					continue;
				#pragma unroll
				for (uint32_t kind = 0; kind < 3; ++kind)
				{
					if (((flags >> (2u * kind)) & 3u) != k_sub_track_animated)
						continue;
					const float3 v = search_value(source, track, kind, rate, at.start + sample);
					if (kind == 0)
						rotation_table[index] = search_rotation_of(v);
					else
					{
						vector_table[kind - 1u][index * 3u] = v.x;
						vector_table[kind - 1u][index * 3u + 1u] = v.y;
						vector_table[kind - 1u][index * 3u + 2u] = v.z;
					}
				}
			}
			[[maybe_unused]] compress_additive_base additive = {};
			[[maybe_unused]] qvv own_base = {};			// (kAdditive: the base sample that goes with sample `lane` of the segment)
			if constexpr (kAdditive)
			{
				additive = compress_additive_base_of(base, instance, raw);
				own_base = search_base_local(additive, track, compress_base_key(additive, at.start + (lane < at.count ? lane : 0u)));
			}
			if (lane < at.count)
			{
				qvv local = search_raw_local(source, track, at.start + lane);
				if constexpr (kAdditive)
					local = search_apply_additive(has_scale, additive, own_base, local);
				float* out = raw_table + lane * 10u;
				out[0] = local.rotation.x; out[1] = local.rotation.y; out[2] = local.rotation.z; out[3] = local.rotation.w;
				out[4] = local.translation.x; out[5] = local.translation.y; out[6] = local.translation.z;
				out[7] = local.scale.x; out[8] = local.scale.y; out[9] = local.scale.z;
			}
			__syncthreads();

			const float4 nothing = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			const float4 fixed_rotation = animated_rotation ? nothing : search_fixed_value(source, track, 0, flags & 3u);
			const float4 fixed_translation = animated_translation ? nothing : search_fixed_value(source, track, 1, (flags >> 2) & 3u);
			const float4 fixed_scale = ((flags >> 4) & 3u) == k_sub_track_animated ? nothing : search_fixed_value(source, track, 2, (flags >> 4) & 3u);

			const uint32_t* list = num_kinds == 1 ? k_search_permutations_1.entries : num_kinds == 2 ? k_search_permutations_2.entries : k_search_permutations_3.entries;
			const uint32_t list_size = num_kinds == 1 ? 25u : num_kinds == 2 ? 625u : 15625u;
			const uint32_t initial = source.multiple ? 0u : 1u;
			uint32_t best = k_search_invalid_rates;
			#pragma unroll
			for (uint32_t k = 0; k < 3; ++k)
				if (k < num_kinds)
					best = (best & ~(0xFFu << (8u * kinds[k]))) | (initial << (8u * kinds[k]));
			float best_error = 1.0e10f;
			uint32_t position = 0, previous_size = 0xFFFFFFFFu;
			while (position < list_size)
			{
				const uint32_t size = list[position] >> 24;
				if (best_error < shell.y && size != previous_size)
					break;				// good enough: the sizes behind that one are not tried
				previous_size = size;
				const uint32_t entry = position + lane < list_size ? list[position + lane] : 0xFFFFFFFFu;
				const bool in_class = (entry >> 24) == size;
				position += uint32_t(__popcll(__ballot(in_class)));

				uint32_t rates = k_search_invalid_rates;
				bool tried = in_class;
				#pragma unroll
				for (uint32_t k = 0; k < 3; ++k)
					if (k < num_kinds)
					{
						const uint32_t rate = (entry >> (8u * k)) & 0xFFu;
						tried = tried && (source.multiple || rate != 0);		// 0 bits need a segment range
						rates = (rates & ~(0xFFu << (8u * kinds[k]))) | (rate << (8u * kinds[k]));
					}
				float error = 0.0f;
				if (tried)
				{
					for (uint32_t sample = 0; sample < at.count; ++sample)
					{
						const float* in = raw_table + sample * 10u;
						qvv raw_local, lossy;
						raw_local.rotation = make_float4(in[0], in[1], in[2], in[3]);
						raw_local.translation = make_float4(in[4], in[5], in[6], 0.0f);
						raw_local.scale = make_float4(in[7], in[8], in[9], 0.0f);
						const uint32_t r = (rates & 0xFFu) * at.count + sample, t = ((rates >> 8) & 0xFFu) * at.count + sample, s = ((rates >> 16) & 0xFFu) * at.count + sample;
						lossy.rotation = (flags & 3u) == k_sub_track_animated ? rotation_table[r] : fixed_rotation;
						lossy.translation = ((flags >> 2) & 3u) == k_sub_track_animated ? make_float4(vector_table[0][t * 3u], vector_table[0][t * 3u + 1u], vector_table[0][t * 3u + 2u], 0.0f) : fixed_translation;
						lossy.scale = ((flags >> 4) & 3u) == k_sub_track_animated ? make_float4(vector_table[1][s * 3u], vector_table[1][s * 3u + 1u], vector_table[1][s * 3u + 2u], 0.0f) : fixed_scale;
						if constexpr (kAdditive)
						{
							// (a lane that has left the scan has left this loop: `sample` is one value over the lanes that are here)
							const int from = int(__builtin_amdgcn_readfirstlane(sample));
							const auto of_lane = [&](float value) __attribute__((always_inline)) -> float { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(value), from)); };
							qvv base_local;
							base_local.rotation = make_float4(of_lane(own_base.rotation.x), of_lane(own_base.rotation.y), of_lane(own_base.rotation.z), of_lane(own_base.rotation.w));
							base_local.translation = make_float4(of_lane(own_base.translation.x), of_lane(own_base.translation.y), of_lane(own_base.translation.z), 0.0f);
							base_local.scale = make_float4(of_lane(own_base.scale.x), of_lane(own_base.scale.y), of_lane(own_base.scale.z), 0.0f);
							lossy = search_apply_additive(has_scale, additive, base_local, lossy);
						}
						const float sample_error = search_error<kMetric>(has_scale, shell.x, raw_local, lossy);
						error = sample_error > error ? sample_error : error;
						if (sample_error >= shell.y)
							break;
					}
				}
				// (smallest error, first lane that has it) over the lanes that tried
				float lowest = tried ? error : __builtin_inff();
				uint32_t lowest_lane = tried ? lane : 0xFFFFFFFFu;
				#pragma unroll
				for (int offset = int(k_wave_size) / 2; offset != 0; offset >>= 1)
				{
					const float other = __shfl_xor(lowest, offset);
					const uint32_t other_lane = uint32_t(__shfl_xor(int(lowest_lane), offset));
					const bool take = other < lowest || (other == lowest && other_lane < lowest_lane);
					lowest = take ? other : lowest;
					lowest_lane = take ? other_lane : lowest_lane;
				}
				lowest_lane = __builtin_amdgcn_readfirstlane(lowest_lane);
				if (lowest_lane != 0xFFFFFFFFu)
				{
					const float found = __shfl(lowest, int(lowest_lane));
					const uint32_t found_rates = uint32_t(__shfl(int(rates), int(lowest_lane)));
					if (found < best_error)
					{
						best_error = found;
						best = found_rates;
					}
				}
			}
			if (lane == 0)
				*row = best;
		}
	}

	// ---- per instance: the level that is searched (aclhip_find_bit_rates_level_batch) ---------------------------------------------------------------
	// Behind the segment launch, which has written the instance's status: an instance that is served gets its level, 0 .. 4, in the second
	// word of its result, where the object phase reads it; any other keeps the 0. ACLHIP_LEVEL_AUTOMATIC is find_best_compression_level
	// (compress.transform.impl.h:114-136) per instance: medium above 500 samples -- the count as registered: the reference resolves the
	// level before its looping vote --, else by the longest chain in bones from a root to a leaf over the instance's tracks (lanes <->
	// tracks; a parent lies in front of its child, or the instance was refused: every walk ends): below 18 highest, below 25 high.
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void bit_rate_search_level_kernel(bit_rate_search_levels_launch launch)
	{
		const transform_compress_launch& base = launch.search.variable.base;
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t instance = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		if (instance >= base.num_instances || base.results[instance].x != ACLHIP_COMPRESS_OK)
			return;
		uint32_t level = launch.level;
		if (level == ACLHIP_LEVEL_AUTOMATIC)
		{
			const uint32_t handle = as_constant(base.raws)[instance];
			const device_raw_tracks raw = load_raw_tracks_fields(base.arrays, handle < base.num_arrays ? handle : 0);
			level = 2;
			if (raw.num_samples <= 500)
			{
				uint32_t longest = 0;
				for (uint32_t track = lane; track < raw.num_tracks; track += k_wave_size)
				{
					uint32_t links = 1;
					for (uint32_t up = compress_track_parent(base, track, raw.num_tracks); up != ACLHIP_NO_PARENT; up = compress_track_parent(base, up, raw.num_tracks))
						++links;
					longest = links > longest ? links : longest;
				}
				#pragma unroll
				for (int offset = int(k_wave_size) / 2; offset != 0; offset >>= 1)
				{
					const uint32_t other = uint32_t(__shfl_xor(int(longest), offset));
					longest = other > longest ? other : longest;
				}
				level = longest < 18 ? 4u : longest < 25 ? 3u : 2u;
			}
		}
		if (lane == 0)
			base.results[instance].y = level;
	}

	// ---- per (instance, segment): the object phase -------------------------------------------------------------------------------------------------
	// S4, loop for loop (quantize.transform.h:997-1098, 1227-1475). Every loop ends. The first one raises one rate of the chain by one in
	// every round that goes on, and a rate stops at 24. The last pass may LOWER rates again (a link keeps the rates of its lowest error,
	// its own at the start included), but every link leaves its inner loop either below the threshold, which ends the pass, or maxed
	// out, and when every link was maxed out the pass ends too: its outer loop runs once. One wave64, lanes <-> the segment's samples
	// (31 at most). An object
	// error walks the chain of its target from the root per lane, the raw transforms beside the lossy ones, and ends in a ballot (the
	// first sample whose error is too high) and a butterfly: every decision is wave uniform. A candidate is the table with ONE track's
	// rates replaced: nothing is copied. The first version recomputes the whole chain for every candidate. Under the matrix metric
	// (kMetric) a segment with scale takes both chains down as 3x4 matrices, 24 floats a lane; without scale it is the qvvf walk.
	// kAdditive: where a link's two local transforms are made, both go through A with the link's base sample (search_base_local at the
	// lane's key) before the walk down the chain: A(raw) is made there once per (link, sample), beside the raw transform it comes from.
	template<uint32_t kMetric, bool kLevels = false, bool kAdditive = false>
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void bit_rate_search_object_kernel(std::conditional_t<kLevels, bit_rate_search_levels_launch, bit_rate_search_launch> record)
	{
		const bit_rate_search_launch& launch = search_launch_of(record);
		const transform_compress_launch& base = launch.variable.base;
		const uint32_t max_segments = launch.variable.max_segments;
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint64_t num_waves = uint64_t(base.num_instances) * max_segments;
		for (uint64_t wave = uint64_t(blockIdx.x) * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size); wave < num_waves;
			wave += uint64_t(gridDim.x) * k_compress_waves_per_block)
		{
			const search_segment at = launch.segments[wave];
			if (at.valid == 0)
				continue;
			const uint32_t instance = uint32_t(wave / max_segments), segment = uint32_t(wave % max_segments);
			const compress_instance voted = load_compress_instance(base.instances, instance);
			const uint32_t handle = as_constant(base.raws)[instance];
			const device_raw_tracks raw = load_raw_tracks_fields(base.arrays, handle < base.num_arrays ? handle : 0);
			const uint32_t num_tracks = voted.num_tracks;
			const uint8_t* track_flags = base.track_flags + size_t(instance) * base.max_tracks;
			const float2* shells = launch.segment_shells + wave * base.max_tracks;
			uint16_t* chain = launch.chains + wave * base.max_tracks;
			uint32_t* row = reinterpret_cast<uint32_t*>(launch.table + instance * launch.instance_stride + segment * launch.segment_stride);
			const bool has_scale = at.has_scale != 0;
			const uint32_t sample = lane < at.count ? lane : 0u;
			// the level that is searched: bit_rate_search_level_kernel left it in the instance's result
			[[maybe_unused]] uint32_t level = 0;
			if constexpr (kLevels)
				level = __builtin_amdgcn_readfirstlane(base.results[instance].y);

			search_source source;
			source.samples = raw.samples;
			source.pose_quads = size_t(num_tracks) * 3u;
			source.clip_ranges = launch.variable.clip_ranges + size_t(instance) * base.max_tracks * k_variable_range_floats;
			source.segment_ranges = launch.segment_ranges + wave * base.max_tracks * k_search_segment_floats;
			source.default_pose = base.default_pose;
			source.start = at.start;
			source.count = at.count;
			source.multiple = variable_split_of(voted.num_out_samples).num_segments > 1;
			[[maybe_unused]] compress_additive_base additive = {};
			[[maybe_unused]] uint32_t base_key = 0;
			if constexpr (kAdditive)
			{
				additive = compress_additive_base_of(base, instance, raw);
				base_key = compress_base_key(additive, at.start + sample);
			}

			const auto parent_of = [&](uint32_t track) -> uint32_t { return compress_track_parent(base, track, num_tracks); };
			const uint32_t none = ACLHIP_NO_PARENT;

			// S2: the object error of chain[links - 1] with the rates of `replaced` taken from `replacement` (with the levels: of up to three
			// tracks; a place that is not used names no track)
			const auto candidate_error = [&](uint32_t links, uint32_t replaced, uint32_t replacement, uint32_t replaced_1, uint32_t replacement_1, uint32_t replaced_2,
				uint32_t replacement_2, bool until_end) __attribute__((always_inline)) -> float
			{
				float2 shell;
				float error = 0.0f;
				bool measured = false;
				if constexpr (kMetric == k_metric_matrix)
				{
					// the matrix metric with scale: O_0 = M(L_0), O_k = matrix_mul(M(L_k), O_k-1), nothing normalized (transform_error_metrics.h:415-436);
					// two matrices, 24 floats, go down the chain where the qvvf metric takes two QVVs
					if (has_scale)
					{
						matrix3x4 raw_object, lossy_object;
						for (uint32_t link = 0; link < links; ++link)
						{
							const uint32_t track = chain[link];
							uint32_t rates = track == replaced ? replacement : row[track];
							if constexpr (kLevels)
								rates = track == replaced_1 ? replacement_1 : track == replaced_2 ? replacement_2 : rates;
							const matrix3x4 lossy_local = matrix_from_qvv(search_lossy_local(source, track, track_flags[track], rates, sample));
							const matrix3x4 raw_local = matrix_from_qvv(search_raw_local(source, track, at.start + sample));
							raw_object = link == 0 ? raw_local : matrix_mul(raw_local, raw_object);
							lossy_object = link == 0 ? lossy_local : matrix_mul(lossy_local, lossy_object);
						}
						shell = shells[chain[links - 1u]];
						error = lane < at.count ? matrix_shell_error(shell.x, raw_object, lossy_object) : 0.0f;
						measured = true;
					}
				}
				if (!measured)
				{
					qvv raw_object, lossy_object;
					for (uint32_t link = 0; link < links; ++link)
					{
						const uint32_t track = chain[link];
						uint32_t rates = track == replaced ? replacement : row[track];
						if constexpr (kLevels)
							rates = track == replaced_1 ? replacement_1 : track == replaced_2 ? replacement_2 : rates;
						qvv lossy_local = search_lossy_local(source, track, track_flags[track], rates, sample);
						qvv raw_local = search_raw_local(source, track, at.start + sample);
						if constexpr (kAdditive)
						{
							const qvv base_local = search_base_local(additive, track, base_key);
							raw_local = search_apply_additive(has_scale, additive, base_local, raw_local);
							lossy_local = search_apply_additive(has_scale, additive, base_local, lossy_local);
						}
						raw_object = link == 0 ? raw_local : search_to_object(has_scale, raw_local, raw_object);
						lossy_object = link == 0 ? lossy_local : search_to_object(has_scale, lossy_local, lossy_object);
					}
					shell = shells[chain[links - 1u]];
					error = lane < at.count ? search_error<kMetric>(has_scale, shell.x, raw_object, lossy_object) : 0.0f;
				}
				if (!until_end)
				{
					const uint64_t high = __ballot(lane < at.count && error >= shell.y);
					if (high != 0)
						error = lane <= uint32_t(__ffsll((long long)high)) - 1u ? error : 0.0f;
				}
				return compress_wave_max(error);
			};
			const auto object_error = [&](uint32_t links, uint32_t replaced, uint32_t replacement, bool until_end) __attribute__((always_inline)) -> float
			{
				return candidate_error(links, replaced, replacement, none, 0, none, 0, until_end);
			};

			const auto increment = [](uint32_t rate, uint32_t by) -> uint32_t
			{
				const uint32_t sum = rate + by;
				return rate >= k_variable_raw_rate ? rate : sum < k_variable_raw_rate ? sum : k_variable_raw_rate;
			};

			// increase_bone_bit_rate with `by` increments (one without the levels): the error is measured AT chain[link], the chain bone
			// whose rate is being tried
			const auto increase_bone_bit_rate = [&](uint32_t link, uint32_t by, float old_error) -> uint32_t
			{
				const uint32_t track = chain[link];
				const uint32_t rates = row[track];
				const uint32_t rotation_rate = rates & 0xFFu, translation_rate = (rates >> 8) & 0xFFu, scale_rate = (rates >> 16) & 0xFFu;
				uint32_t best = rates;
				float best_error = old_error;
				for (uint32_t rotation_increment = 0; rotation_increment <= by; ++rotation_increment)
				{
					const uint32_t rotation = increment(rotation_rate, rotation_increment);
					for (uint32_t translation_increment = 0; translation_increment <= by; ++translation_increment)
					{
						const uint32_t translation = increment(translation_rate, translation_increment);
						for (uint32_t scale_increment = 0; scale_increment <= (has_scale ? by : 0u); ++scale_increment)
						{
							const uint32_t scale = increment(scale_rate, scale_increment);
							if (rotation_increment + translation_increment + scale_increment != by)
							{
								if (scale >= k_variable_raw_rate)
									break;
								continue;
							}
							const uint32_t tried = rotation | (translation << 8) | (scale << 16);
							const float error = object_error(link + 1u, track, tried, false);
							if (error < best_error)
							{
								best_error = error;
								best = tried;
							}
							if (scale >= k_variable_raw_rate)
								break;
						}
						if (translation >= k_variable_raw_rate)
							break;
					}
					if (rotation >= k_variable_raw_rate)
						break;
				}
				return best;
			};

			const auto search_track = [&](uint32_t track)
			{
				// the chain, from the root: every lane stores the same entries and reads its own
				uint32_t links = 1;
				for (uint32_t up = parent_of(track); up != ACLHIP_NO_PARENT; up = parent_of(up))
					++links;
				{
					uint32_t at_link = links;
					for (uint32_t up = track; up != ACLHIP_NO_PARENT; up = parent_of(up))
						chain[--at_link] = uint16_t(up);
				}
				const float threshold = shells[track].y;

				float error = object_error(links, none, 0, false);
				if (error < threshold)
					return;
				const float initial_error = error;
				if constexpr (!kLevels)
				{
					uint32_t best_track = none, best_rates = 0;
					while (error >= threshold)
					{
						const float original_error = error;
						float best_error = error;
						// calculate_bone_permutation_error for "one increment somewhere in the chain": own track first, then toward the root
						uint32_t found_track = none, found_rates = 0;
						float found_error = original_error;
						for (uint32_t link = links; link-- != 0;)
						{
							const uint32_t chain_track = chain[link];
							const uint32_t tried = increase_bone_bit_rate(link, 1, original_error);
							if (tried == row[chain_track])
								continue;
							const float permutation_error = object_error(links, chain_track, tried, false);
							if (permutation_error < found_error)
							{
								found_error = permutation_error;
								found_track = chain_track;
								found_rates = tried;
								if (permutation_error < threshold)
									break;
							}
						}
						error = found_error;
						if (error < best_error)
						{
							best_error = error;
							best_track = found_track;
							best_rates = found_rates;
							if (error < threshold)
								break;
						}
						if (best_error >= original_error)
							break;				// no progress
						error = best_error;
						row[best_track] = best_rates;
					}
					if (error < initial_error)
						row[best_track] = best_rates;
				}
				else
				{
					// The first loop with the levels (quantize.transform.h:1250-1377). A round's bar is original_error throughout and best_error is
					// carried across its calls of calculate_bone_permutation_error, one per SHAPE of increments over the chain:
					//   every level  {1} on one link (the loop above)
					//   >= high      {2} on one link; with more than one link {1,1} on two
					//   >= highest   {3} on one link; with more than one link {2,1}; with more than two {1,1,1}
					// After a call: error < best_error keeps that permutation's rates, and error < threshold leaves the round. A shape's
					// arrangements come in std::next_permutation order over the chain array, root first -- the own track changes fastest --,
					// which the positions a > b > c below count down: no array is permuted. What to keep in mind:
					//   1. {2,1} STARTS at [..., 2, 1], parent + 2 and own + 1, which is not its smallest arrangement: next_permutation runs
					//      from there to the end, so [..., 1, 2] is never tried and a chain of two links tries exactly one arrangement. Every
					//      other shape starts at its smallest arrangement and visits all of them.
					//   2. increase_bone_bit_rate(link, n) enumerates the (rotation, translation, scale) increments that sum to n with the
					//      reference's break and continue rules at rate 24; without scale the scale's is 0. It measures at the chain bone
					//      whose rate is tried, not at the track under work, and its bar is old_error, the round's original_error.
					//   3. A permutation counts only if one of its links changed its rates (is_permutation_valid): an invalid one is skipped
					//      without measuring.
					//   4. Inside one call a permutation below the threshold ends that call at once.
					//   5. A candidate is the table with up to three tracks' rates replaced: nothing is copied.
					// THE MEMO. Within a round neither the rates nor original_error change, so increase_bone_bit_rate(link, n) depends on (link, n)
					// alone. The reference recomputes it for every arrangement; here it is computed when an arrangement first asks for it and
					// kept, three dwords per link (k_search_memo_unset: not asked yet), in the workspace: every lane stores the same dword and
					// reads its own. No decision sees the difference. Every loop ends: a shape has finitely many arrangements, each visited
					// once; a round that goes on has lowered the error by raising at least one rate, and rates stop at 24.
					uint32_t* memo = record.memo + wave * base.max_tracks * 3u;
					uint32_t best_tracks[3] = { none, none, none }, best_rates[3] = { 0, 0, 0 };
					const auto apply_best = [&]()
					{
						#pragma unroll
						for (uint32_t k = 0; k < 3; ++k)
							if (best_tracks[k] != none)
								row[best_tracks[k]] = best_rates[k];
					};
					while (error >= threshold)
					{
						const float original_error = error;
						float best_error = error;
						for (uint32_t index = 0; index < links * 3u; ++index)
							memo[index] = k_search_memo_unset;
						bool met = false;
						// the shapes in the reference's order: {1}, {2}, {1,1}, {3}, {2,1}, {1,1,1}
						for (uint32_t shape = 0; shape < 6 && !met; ++shape)
						{
							const uint32_t shape_links = shape == 2 || shape == 4 ? 2u : shape == 5 ? 3u : 1u;
							if (level < (shape == 0 ? 0u : shape < 3 ? 3u : 4u) || links < shape_links)
								continue;
							// calculate_bone_permutation_error. The links that carry an increment are a > b > c (the root is link 0); of {2,1}
							// b, the link nearer the root, carries the 2 and a the 1 while `parent_two`, else b the 1 and a the 2.
							uint32_t a = links - 1u, b = links - 2u, c = links - 3u;
							bool parent_two = shape == 4;		// (trap 1: the start)
							uint32_t found_tracks[3] = { none, none, none }, found_rates[3] = { 0, 0, 0 };
							float found_error = original_error;
							for (;;)
							{
								const uint32_t increment_a = shape == 1 ? 2u : shape == 3 ? 3u : shape == 4 && !parent_two ? 2u : 1u;
								const uint32_t increment_b = shape_links < 2 ? 0u : shape == 4 && parent_two ? 2u : 1u;
								const uint32_t increment_c = shape_links < 3 ? 0u : 1u;
								// what the memo lacks of this arrangement, root first
								#pragma nounroll
								for (uint32_t k = 3; k-- != 0;)
								{
									const uint32_t link = k == 0 ? a : k == 1 ? b : c, by = k == 0 ? increment_a : k == 1 ? increment_b : increment_c;
									if (by == 0)
										continue;
									if (__builtin_amdgcn_readfirstlane(memo[link * 3u + by - 1u]) == k_search_memo_unset)
										memo[link * 3u + by - 1u] = increase_bone_bit_rate(link, by, original_error);
								}
								uint32_t tried_tracks[3] = { chain[a], none, none }, tried_rates[3] = { memo[a * 3u + increment_a - 1u], 0, 0 };
								if (increment_b != 0)
								{
									tried_tracks[1] = chain[b];
									tried_rates[1] = memo[b * 3u + increment_b - 1u];
								}
								if (increment_c != 0)
								{
									tried_tracks[2] = chain[c];
									tried_rates[2] = memo[c * 3u + increment_c - 1u];
								}
								bool valid = false;
								#pragma unroll
								for (uint32_t k = 0; k < 3; ++k)
									valid = valid || (tried_tracks[k] != none && tried_rates[k] != row[tried_tracks[k] != none ? tried_tracks[k] : 0u]);
								if (__builtin_amdgcn_readfirstlane(uint32_t(valid)) != 0)
								{
									const float permutation_error = candidate_error(links, tried_tracks[0], tried_rates[0], tried_tracks[1], tried_rates[1], tried_tracks[2], tried_rates[2], false);
									if (permutation_error < found_error)
									{
										found_error = permutation_error;
										#pragma unroll
										for (uint32_t k = 0; k < 3; ++k)
										{
											found_tracks[k] = tried_tracks[k];
											found_rates[k] = tried_rates[k];
										}
										if (permutation_error < threshold)
											break;
									}
								}
								// the next arrangement: the lowest link steps toward the one above it, then that one steps and the lower ones start
								// again at the own track's end; {2,1} goes through "b carries the 1" before "b carries the 2" at every b but the first
								if (shape_links == 1)
								{
									if (a == 0)
										break;
									--a;
								}
								else if (shape_links == 2)
								{
									if (a > b + 1u)
										--a;
									else if (shape == 4 && !parent_two)
									{
										parent_two = true;
										a = links - 1u;
									}
									else if (b == 0)
										break;
									else
									{
										--b;
										a = links - 1u;
										parent_two = false;
									}
								}
								else
								{
									if (a > b + 1u)
										--a;
									else if (b > c + 1u)
									{
										--b;
										a = links - 1u;
									}
									else if (c == 0)
										break;
									else
									{
										--c;
										b = links - 2u;
										a = links - 1u;
									}
								}
							}
							error = found_error;
							if (error < best_error)
							{
								best_error = error;
								#pragma unroll
								for (uint32_t k = 0; k < 3; ++k)
								{
									best_tracks[k] = found_tracks[k];
									best_rates[k] = found_rates[k];
								}
								met = error < threshold;
							}
						}
						if (met)
							break;
						if (best_error >= original_error)
							break;				// no progress
						error = best_error;
						apply_best();
					}
					if (error < initial_error)
						apply_best();
				}

				// the error remains too high: from child to parent, increase indiscriminately and keep the best
				error = object_error(links, none, 0, true);
				while (error >= threshold)
				{
					uint32_t num_maxed_out = 0;
					for (uint32_t link = links; link-- != 0;)
					{
						const uint32_t chain_track = chain[link];
						uint32_t rates = row[chain_track];
						uint32_t best_link_rates = rates;
						float best_link_error = error;
						while (error >= threshold)
						{
							const uint32_t rotation = rates & 0xFFu, translation = (rates >> 8) & 0xFFu, scale = (rates >> 16) & 0xFFu;
							// std::min_element: the first of the smallest
							const uint32_t smallest = translation < rotation ? (scale < translation ? 2u : 1u) : (scale < rotation ? 2u : 0u);
							const uint32_t smallest_rate = smallest == 0 ? rotation : smallest == 1 ? translation : scale;
							if (smallest_rate >= k_variable_raw_rate)
							{
								++num_maxed_out;
								break;
							}
							if (rotation == translation && translation < k_variable_raw_rate && scale >= k_variable_raw_rate)
								rates += 1u << 8;
							else
								rates += 1u << (8u * smallest);
							row[chain_track] = rates;
							error = object_error(links, none, 0, true);
							if (error < best_link_error)
							{
								best_link_rates = rates;
								best_link_error = error;
							}
						}
						row[chain_track] = best_link_rates;
						error = best_link_error;
						if (error < threshold)
							break;
					}
					if (num_maxed_out == links)
						break;
				}
				// (the reference's last pass, which maxes the rates out, is for quatf_full alone: never here)
			};

			// sorted_transforms_parent_first (clip_context.impl.h:57-80): by parent + 1 in 32 bits -- the roots first --, then by own index
			for (uint32_t key = 0; key <= num_tracks; ++key)
			{
				const uint32_t wanted = key == 0 ? ACLHIP_NO_PARENT : key - 1u;
				for (uint32_t first = key == 0 ? 0u : key; first < num_tracks; first += k_wave_size)
				{
					const uint32_t track = first + lane;
					uint64_t matches = __ballot(track < num_tracks && parent_of(track < num_tracks ? track : 0u) == wanted);
					while (matches != 0)
					{
						const uint32_t bit = uint32_t(__ffsll((long long)matches)) - 1u;
						matches &= matches - 1u;
						search_track(first + bit);
					}
				}
			}
		}
	}
