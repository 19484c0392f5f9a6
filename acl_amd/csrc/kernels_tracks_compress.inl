// kernels_tracks_compress.inl -- part of aclhip.hip (one translation unit; included there behind kernels_transform_compress.inl, not compiled on its own).
// aclhip_compress_tracks_batch with rotation_format = quatf_drop_w_full: what the reference's compress_track_list does once the rotation
// format is not quatf_full and nothing is variable (compression/impl/compress.transform.impl.h:138-530) -- rotations normalized, the rigid
// shell of every transform from the hierarchy, the looping vote and the constant and default rotation sub-tracks by the error metric at
// that shell, 96 bit rotations. Five stream ordered launches:
//   tracks_compress_shell_kernel       per instance: the refusals, the finite test, the rigid shell, the looping vote
//   tracks_compress_analyze_kernel     per (instance, track): the two shell error ballots of the rotation, the binary tests of translation
//                                      and scale: one flag byte per track, no atomics
//   transform_compress_layout_kernel<true>, transform_compress_stream_kernel<true>   (kernels_transform_compress.inl) with three words per rotation
//   compress_hash_kernel               (kernels_scalar_compress.inl)
// include/aclhip.h states the definition: fp32, one IEEE operation at a time; shell_error and qvv_mul_point3 are the pose error kernel's
// (kernels_pose_buffers.inl). The shell kernel and the analysis take the error metric of their decisions as a template argument
// (aclhip_compress_tracks_metric_batch): compress_shell_error, below; and, beside it, whether the instance is an additive clip that is
// decided on its base (aclhip_compress_tracks_additive_batch): compress_additive_base, below.

	constexpr uint32_t k_compress_optimize_loops = 1;				// ACLHIP_COMPRESS_OPTIMIZE_LOOPS

	// sample `sample` of track `track` as the metric sees it: the rotation normalized (not yet of positive w), the fourth lanes 0
	__device__ __forceinline__ qvv tracks_compress_sample(const f32x4* samples, size_t pose_quads, uint32_t sample, uint32_t track)
	{
		const f32x4* record = samples + sample * pose_quads + size_t(track) * 3u;
		const f32x4 q = record[0], t = record[1], s = record[2];
		qvv result;
		result.rotation = tracks_compress_normalize(q);
		result.translation = make_float4(t.x, t.y, t.z, 0.0f);
		result.scale = make_float4(s.x, s.y, s.z, 0.0f);
		return result;
	}

	// the ten used lanes of a sample, the rotation as normalized
	__device__ __forceinline__ bool tracks_compress_finite(const qvv& transform)
	{
		return transform_compress_finite(transform.rotation.x) && transform_compress_finite(transform.rotation.y) && transform_compress_finite(transform.rotation.z)
			&& transform_compress_finite(transform.rotation.w)
			&& transform_compress_finite(transform.translation.x) && transform_compress_finite(transform.translation.y) && transform_compress_finite(transform.translation.z)
			&& transform_compress_finite(transform.scale.x) && transform_compress_finite(transform.scale.y) && transform_compress_finite(transform.scale.z);
	}

	__device__ __forceinline__ float tracks_compress_length3(float4 v) { return sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z); }

	// the largest value of the wave, the same in every lane (a butterfly; no value is a NaN inside the definition, so the order of the
	// steps does not show)
	__device__ __forceinline__ float compress_wave_max(float value)
	{
		#pragma unroll
		for (int offset = int(k_wave_size) / 2; offset != 0; offset >>= 1)
		{
			const float other = __shfl_xor(value, offset);
			value = other > value ? other : value;
		}
		return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(value)));
	}

	// The error a compressor's decisions are taken by, per aclhip_error_metric (a template argument of the kernels that decide: the qvvf
	// instantiations are the kernels without it): qvvf_transform_error_metric's shell_error, or qvvf_matrix3x4f_transform_error_metric's
	// -- both transforms through matrix_from_qvv, then matrix_shell_error (kernels_pose_buffers.inl; transform_error_metrics.h:389-461).
	constexpr uint32_t k_metric_qvvf = 0, k_metric_matrix = 1;		// ACLHIP_METRIC_QVVF, ACLHIP_METRIC_QVVF_MATRIX3X4F
	template<uint32_t kMetric>
	__device__ __forceinline__ float compress_shell_error(float distance, const qvv& raw, const qvv& lossy)
	{
		if constexpr (kMetric == k_metric_matrix)
			return matrix_shell_error(distance, matrix_from_qvv(raw), matrix_from_qvv(lossy));
		else
			return shell_error(distance, raw, lossy);
	}

	// ---- additive bases (the _additive entry points) ------------------------------------------------------------------------------------------
	// An additive clip's decisions are taken after it has been applied onto its base (additive_qvvf_transform_error_metric<format>,
	// transform_error_metrics.h:469-524): the kernels that decide take kAdditive as a template argument, beside the metric, and the
	// instantiations without it are the kernels as they were. Nothing of the base is stored: a base sample is read where it is used.
	// What a kernel holds of an instance's base, all wave uniform:
	struct compress_additive_base
	{
		const f32x4* samples;			// the base's records
		size_t pose_quads;				// of one of its key frames
		uint32_t num_samples;
		float sample_rate, duration;	// the base's own
		float clip_rate, clip_duration;	// the instance's, as registered
		uint32_t format;				// an aclhip_additive_format, not 0
	};

	__device__ __forceinline__ compress_additive_base compress_additive_base_of(const transform_compress_launch& launch, const device_raw_tracks& raw, const device_raw_tracks& base)
	{
		compress_additive_base out;
		out.samples = base.samples;
		out.pose_quads = size_t(base.num_tracks) * 3u;
		out.num_samples = base.num_samples;
		out.sample_rate = base.sample_rate;
		out.duration = base.duration;
		out.clip_rate = raw.sample_rate;
		out.clip_duration = raw.duration;
		out.format = launch.additive_format;
		return out;
	}
	// (behind the shell kernel, which has refused every instance whose base is no live array or has too few tracks)
	__device__ __forceinline__ compress_additive_base compress_additive_base_of(const transform_compress_launch& launch, uint32_t instance, const device_raw_tracks& raw)
	{
		const uint32_t handle = as_constant(launch.base_raws)[instance];
		return compress_additive_base_of(launch, raw, load_raw_tracks_fields(launch.arrays, handle < launch.num_arrays ? handle : 0));
	}

	// The base's key that goes with sample `sample` of the clip: the time min(sample / rate, D) of the clip, scaled by D_b / D onto the
	// base, then get_uniform_sample_key (sample_streams.h:557-601): find_linear_interpolation_samples_with_sample_rate with
	// sample_rounding_policy::nearest, never looping, over the base's own count and rate. The base is never interpolated. A clip of one
	// sample has D = 0 and the time is 0 / 0: the reference's conversion of that NaN gives key 0 and its alpha fails `== 0`: the key
	// after it, stated here as such. A key behind the last (no time inside the definition gives one) is the last.
	__device__ __forceinline__ uint32_t compress_base_key(const compress_additive_base& base, uint32_t sample)
	{
		if (base.num_samples <= 1)
			return 0;
		const uint32_t last = base.num_samples - 1u;
		const float time = float(sample) / base.clip_rate;
		const float sample_time = time < base.clip_duration ? time : base.clip_duration;
		const float sample_index = ((sample_time / base.clip_duration) * base.duration) * base.sample_rate;
		if (!(sample_index == sample_index))
			return 1u < last ? 1u : last;
		const uint32_t index0 = uint32_t(sample_index);
		const uint32_t key0 = index0 < last ? index0 : last;
		const uint32_t key1 = key0 + 1u < last ? key0 + 1u : last;
		return floorf((sample_index - float(key0)) + 0.5f) == 0.0f ? key0 : key1;
	}

	// base(b, s) at a key: the rotation normalized as the clip's own are (step 1), translation and scale as registered
	__device__ __forceinline__ qvv compress_base_sample(const compress_additive_base& base, uint32_t track, uint32_t key)
	{
		return tracks_compress_sample(base.samples, base.pose_quads, key, track);
	}

	// A(x) = apply_additive_to_base(format, base, x) (core/additive_utils.h:128-162); relative is the quaternion route of qvv_mul
	__device__ __forceinline__ qvv compress_apply_additive(const compress_additive_base& base, const qvv& base_transform, const qvv& additive)
	{
		return apply_additive_to_base<false>(base.format, base_transform, additive);
	}

	// a compaction's shell error: both sides through A with the same base sample; without kAdditive the error itself
	template<uint32_t kMetric, bool kAdditive>
	__device__ __forceinline__ float compress_shell_error_on_base(float distance, const compress_additive_base& base, const qvv& base_transform, const qvv& raw, const qvv& lossy)
	{
		if constexpr (kAdditive)
			return compress_shell_error<kMetric>(distance, compress_apply_additive(base, base_transform, raw), compress_apply_additive(base, base_transform, lossy));
		else
			return compress_shell_error<kMetric>(distance, raw, lossy);
	}

	// ---- per instance: the refusals, the finite test, the rigid shell, the looping vote -----------------------------------------------------
	// One wave64 per instance. The shell (rigid_shell_utils.h:51-170) walks the tracks in DESCENDING order -- every parent index is smaller
	// than its child's, or the instance is refused --, samples across the lanes: a track's stretch is a max over its samples
	// (compress_wave_max), and what it hands to its parent waits in the workspace, { local shell distance, precision } per track: the
	// wave's own stores, read back by the wave itself. Every lane ends a visit with the same numbers, whatever the samples hold. The
	// looping vote (optimize_looping.transform.h:178-243) takes lanes <-> tracks. Leaves status, the sample count behind the vote and
	// the wrap bit in the instance's record: the layout reads them.
	// kAdditive: the refusals and the finite test of the instance's base as well; the stretch over A(sample) with base(b, s); the vote
	// over A_first(first) and A_last(last), the base's sample 0 and its LAST sample (optimize_looping.transform.h:139-163).
	template<uint32_t kMetric, bool kAdditive = false>
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void tracks_compress_shell_kernel(transform_compress_launch launch)
	{
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t instance = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		if (instance >= launch.num_instances)
			return;

		const uint32_t handle = as_constant(launch.raws)[instance];
		const device_raw_tracks raw = load_raw_tracks_fields(launch.arrays, handle < launch.num_arrays ? handle : 0);
		const uint32_t num_tracks = raw.num_tracks;
		const uint32_t num_samples = raw.num_samples;
		float2* shells = launch.shells + size_t(instance) * launch.max_tracks;

		compress_instance record = {};
		bool refused = transform_compress_refused(launch, handle, raw);
		[[maybe_unused]] compress_additive_base base = {};
		if constexpr (kAdditive)
		{
			// a base that is no live raw track array, or has fewer tracks than the instance: the reference would read out of bounds
			const uint32_t base_handle = as_constant(launch.base_raws)[instance];
			const device_raw_tracks base_raw = load_raw_tracks_fields(launch.arrays, base_handle < launch.num_arrays ? base_handle : 0);
			refused = refused || base_handle >= launch.num_arrays || base_raw.samples == nullptr || base_raw.num_samples == 0 || base_raw.num_tracks < num_tracks;
			base = compress_additive_base_of(launch, raw, base_raw);
		}
		if (!refused && launch.parent_indices != nullptr)
		{
			// a parent at or behind its child: the reference's shell would be an artefact of its sort
			bool forward = false;
			for (uint32_t track = lane; track < num_tracks; track += k_wave_size)
			{
				const uint32_t parent = launch.parent_indices[track];
				forward = forward || (parent >= track && parent < num_tracks);
			}
			refused = __ballot(forward) != 0;
		}
		if (refused)
		{
			if (lane == 0)
			{
				record.status = k_compress_status_refused;
				launch.instances[instance] = record;
			}
			return;
		}

		for (uint32_t track = lane; track < num_tracks; track += k_wave_size)
			shells[track] = make_float2(compress_track_shell_distance(launch, track), compress_track_precision(launch, track));

		const size_t pose_quads = size_t(num_tracks) * 3u;
		bool finite = true;
		if constexpr (kAdditive)
		{
			// "Some base samples are not finite": every track and sample of the base, as its own initialize_clip_context sees them
			// (its records lie one behind the other: lanes <-> records)
			const uint64_t base_records = uint64_t(base.pose_quads / 3u) * base.num_samples;
			for (uint64_t index = lane; index < base_records; index += k_wave_size)
				finite = finite && tracks_compress_finite(tracks_compress_sample(base.samples + index * 3u, 0, 0, 0));
		}
		for (uint32_t track = num_tracks; track-- != 0;)
		{
			const float2 shell = shells[track];			// (every lane the same address: what a child's visit stored is what comes back)
			const float distance = shell.x;
			float stretch = 0.0f;
			for (uint32_t sample = lane; sample < num_samples; sample += k_wave_size)
			{
				qvv transform = tracks_compress_sample(raw.samples, pose_quads, sample, track);
				finite = finite && tracks_compress_finite(transform);
				if constexpr (kAdditive)
					transform = compress_apply_additive(base, compress_base_sample(base, track, compress_base_key(base, sample)), transform);
				const float length_x = tracks_compress_length3(qvv_mul_point3(distance, 0.0f, 0.0f, transform));
				const float length_y = tracks_compress_length3(qvv_mul_point3(0.0f, distance, 0.0f, transform));
				const float length_z = tracks_compress_length3(qvv_mul_point3(0.0f, 0.0f, distance, transform));
				stretch = length_x > stretch ? length_x : stretch;
				stretch = length_y > stretch ? length_y : stretch;
				stretch = length_z > stretch ? length_z : stretch;
			}
			stretch = compress_wave_max(stretch);

			const float own_distance = compress_track_shell_distance(launch, track), own_precision = compress_track_precision(launch, track);
			// a transform whose distance a child has raised is not dominant: the error it may add itself comes on top
			const float parent_shell_distance = distance != own_distance ? stretch + own_precision : stretch;
			const uint32_t parent = compress_track_parent(launch, track);
			if (parent < track && parent_shell_distance > shells[parent].x)
				shells[parent] = make_float2(parent_shell_distance, shell.y);
		}

		uint32_t status = __ballot(!finite) != 0 ? k_compress_status_not_finite : 0u;
		uint32_t num_out_samples = num_samples;
		uint32_t wrap = raw.looping_policy == k_loop_wrap ? 1u : 0u;
		if (status == 0 && wrap == 0 && (launch.flags & k_compress_optimize_loops) != 0 && num_samples > 1)
		{
			bool apart = false;
			for (uint32_t track = lane; track < num_tracks; track += k_wave_size)
			{
				const float2 shell = shells[track];
				qvv first = tracks_compress_sample(raw.samples, pose_quads, 0, track), last = tracks_compress_sample(raw.samples, pose_quads, num_samples - 1u, track);
				if constexpr (kAdditive)
				{
					first = compress_apply_additive(base, compress_base_sample(base, track, 0), first);
					last = compress_apply_additive(base, compress_base_sample(base, track, base.num_samples - 1u), last);
				}
				apart = apart || compress_shell_error<kMetric>(shell.x, first, last) > shell.y;
			}
			if (__ballot(apart) == 0)
			{
				num_out_samples = num_samples - 1u;
				wrap = 1;
			}
		}

		if (status == 0 && launch.shell_metadata != nullptr)
		{
			float2* out = launch.shell_metadata + size_t(instance) * launch.max_tracks;
			for (uint32_t track = lane; track < num_tracks; track += k_wave_size)
				out[track] = shells[track];
		}
		if (lane == 0)
		{
			record.num_tracks = num_tracks;
			record.num_samples = num_samples;
			record.num_out_samples = num_out_samples;
			record.wrap = wrap;
			record.status = status;
			launch.instances[instance] = record;
		}
	}

	// ---- per (instance, track): the three sub-track types ---------------------------------------------------------------------------------------
	// transform_compress_analyze_kernel's shape: one wave64 per track, samples across the lanes, over the samples the vote left. The three
	// rotation ballots are two shell error ballots (compact.transform.h:72-254): a sample against sample 0's rotation and against the
	// default rotation, each under the sample's own translation and scale, at the track's shell. Translations and scales as there.
	// kAdditive: both sides of the two shell errors go through A with the sample's base(b, s) (compact.transform.h:168-200).
	template<uint32_t kMetric, bool kAdditive = false>
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void tracks_compress_analyze_kernel(transform_compress_launch launch)
	{
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t track = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		for (uint32_t instance = blockIdx.y; instance < launch.num_instances; instance += gridDim.y)
		{
			const compress_instance voted = load_compress_instance(launch.instances, instance);
			if (voted.status != 0 || track >= voted.num_tracks)
				continue;
			const uint32_t handle = as_constant(launch.raws)[instance];
			const device_raw_tracks raw = load_raw_tracks_fields(launch.arrays, handle < launch.num_arrays ? handle : 0);
			const float2 shell = launch.shells[size_t(instance) * launch.max_tracks + track];

			const size_t pose_quads = size_t(raw.num_tracks) * 3u;
			f32x4 default_rotation = { 0.0f, 0.0f, 0.0f, 1.0f }, default_translation = { 0.0f, 0.0f, 0.0f, 0.0f }, default_scale = { 1.0f, 1.0f, 1.0f, 0.0f };
			if (launch.default_pose != nullptr)
			{
				default_rotation = launch.default_pose[size_t(track) * 3u];
				default_translation = launch.default_pose[size_t(track) * 3u + 1u];
				default_scale = launch.default_pose[size_t(track) * 3u + 2u];
			}
			const qvv first = tracks_compress_sample(raw.samples, pose_quads, 0, track);
			const float4 rotation0 = tracks_compress_positive_w(first.rotation), translation0 = first.translation, scale0 = first.scale;
			[[maybe_unused]] compress_additive_base base = {};
			if constexpr (kAdditive)
				base = compress_additive_base_of(launch, instance, raw);
			bool rotation_moves = false, rotation_leaves_default = false, same_translation = true, same_scale = true;
			for (uint32_t sample = lane; sample < voted.num_out_samples; sample += k_wave_size)
			{
				qvv kept = tracks_compress_sample(raw.samples, pose_quads, sample, track);
				kept.rotation = tracks_compress_positive_w(kept.rotation);
				qvv other = kept;
				other.rotation = rotation0;
				[[maybe_unused]] qvv base_transform = {};
				if constexpr (kAdditive)
					base_transform = compress_base_sample(base, track, compress_base_key(base, sample));
				rotation_moves = rotation_moves || compress_shell_error_on_base<kMetric, kAdditive>(shell.x, base, base_transform, kept, other) > shell.y;
				other.rotation = make_float4(default_rotation.x, default_rotation.y, default_rotation.z, default_rotation.w);
				rotation_leaves_default = rotation_leaves_default || compress_shell_error_on_base<kMetric, kAdditive>(shell.x, base, base_transform, kept, other) > shell.y;
				same_translation = same_translation && kept.translation.x == translation0.x && kept.translation.y == translation0.y && kept.translation.z == translation0.z;
				same_scale = same_scale && kept.scale.x == scale0.x && kept.scale.y == scale0.y && kept.scale.z == scale0.z;
			}
			const bool default_translation_at_0 = translation0.x == default_translation.x && translation0.y == default_translation.y && translation0.z == default_translation.z;
			const bool default_scale_at_0 = scale0.x == default_scale.x && scale0.y == default_scale.y && scale0.z == default_scale.z;

			const uint32_t flags = transform_compress_type(__ballot(rotation_moves) == 0, __ballot(rotation_leaves_default) == 0)
				| (transform_compress_type(__ballot(!same_translation) == 0, default_translation_at_0) << 2)
				| (transform_compress_type(__ballot(!same_scale) == 0, default_scale_at_0) << 4);
			if (lane == 0)
				launch.track_flags[size_t(instance) * launch.max_tracks + track] = uint8_t(flags);
		}
	}
