// kernels_variable_compress.inl -- part of aclhip.hip (one translation unit; included there behind kernels_tracks_compress.inl, not compiled on its own).
// aclhip_compress_tracks_variable_batch: what the reference's compress_track_list does with quatf_drop_w_variable / vector3f_variable /
// vector3f_variable (compression/impl/compress.transform.impl.h:138-530) once the bit rates are known -- everything of the variable
// compressor but find_optimal_bit_rates: the rates are an input. Six stream ordered launches:
//   tracks_compress_shell_kernel         (kernels_tracks_compress.inl, unchanged) the refusals, the finite test, the rigid shell, the vote
//   variable_compress_analyze_kernel     per (instance, track): the six shell error ballots of rotation, translation and scale, each kind
//                                        seeing the kinds compacted before it; the clip ranges of the three kinds: a flag byte and 18 floats
//   variable_compress_layout_kernel      per instance: the segments, per segment the prefix sums of the bit widths in stream order, the
//                                        refusals in front of any write to the row; then everything of the blob but segment ranges and streams
//   variable_compress_ranges_kernel      per (instance, segment), lanes <-> animated sub-tracks: the segment range with the 8 bit fix-up, or
//                                        the 16 bit sample of a sub-track that is constant in the segment
//   variable_compress_stream_kernel      per output dword of a segment's bit stream: the sub-track that reaches into it from the prefix
//                                        sums, every component recomputed from the registered sample and the two ranges, one store
//   compress_hash_kernel                 (kernels_scalar_compress.inl, unchanged)
// include/aclhip.h states the definition: fp32, one IEEE operation at a time. No atomics besides the refusal counter and no zero fill:
// every byte of [0, size) has one writer, the same bytes on every run. aclhip_compress_tracks_variable_additive_batch is these with the
// shell kernel's and the analysis' kAdditive instantiations (kernels_tracks_compress.inl: compress_additive_base); the layout takes the
// header's default-scale bit from the launch record.

	constexpr uint32_t k_variable_raw_rate = 24;				// core/impl/variable_bit_rates.h:45: 32 bits per component; its format byte says 31
	constexpr uint32_t k_variable_raw_format = 31;
	constexpr uint32_t k_variable_ideal_samples = 16;			// compression_settings::segmenting, the reference's defaults
	constexpr uint32_t k_variable_max_samples = 31;
	constexpr uint32_t k_variable_range_floats = 18;			// per track: min xyz, extent xyz of the rotation, the translation, the scale

	// What the layout leaves of a segment for the two launches behind it; offsets from the blob's start
	struct variable_segment
	{
		uint32_t start, count;					// the segment's samples
		uint32_t pose_bits;						// of one sample of its stream
		uint32_t stream_bytes;
		uint32_t formats_at, ranges_at, stream_at;
		uint32_t unused;
	};
	static_assert(sizeof(variable_segment) == 32, "two dwordx4 loads");

	struct variable_compress_launch
	{
		transform_compress_launch base;			// what the shell kernel reads, and every table
		const uint8_t* bit_rates;				// { rotation, translation, scale, 0 } per (instance, segment, track), or null: uniform_rates
		uint64_t bit_rate_instance_stride, bit_rate_segment_stride;
		uint32_t uniform_rates;					// rotation | translation << 8 | scale << 16
		uint32_t max_samples;
		uint32_t max_segments;					// variable_num_segments(max_samples): the rows of the two parts below
		float* clip_ranges;						// [num_instances][max_tracks][18]
		variable_segment* segments;				// [num_instances][max_segments]
		uint32_t* prefix;						// [num_instances][max_segments][3 * max_tracks]: bits of a pose in front of an animated sub-track, in stream order
	};

	// split_samples_per_segment (segment.transform.h:65-128) with 16 ideal and 31 at most, in closed form: up to 31 samples are one
	// segment; else ceil(S / 16) segments of 16 with the rest in the last, and when the others have room for it (15 each) the last one is
	// dealt out over them in turn, one sample at a time.
	struct variable_split { uint32_t num_segments, each, extra, last; bool dealt; };
	__host__ __device__ inline variable_split variable_split_of(uint32_t num_samples)
	{
		variable_split split = { 1, num_samples, 0, num_samples, false };
		if (num_samples <= k_variable_max_samples)
			return split;
		const uint32_t estimated = (num_samples - 1u) / k_variable_ideal_samples + 1u;
		const uint32_t last = num_samples - (estimated - 1u) * k_variable_ideal_samples;		// 1 .. 16
		split.dealt = uint64_t(estimated - 1u) * (k_variable_max_samples - k_variable_ideal_samples) >= last;
		split.num_segments = split.dealt ? estimated - 1u : estimated;
		split.each = k_variable_ideal_samples + (split.dealt ? last / split.num_segments : 0u);
		split.extra = split.dealt ? last % split.num_segments : 0u;
		split.last = last;
		return split;
	}
	__host__ __device__ inline void variable_segment_samples(const variable_split& split, uint32_t segment, uint32_t& start, uint32_t& count)
	{
		start = segment * split.each + (segment < split.extra ? segment : split.extra);
		count = split.each + (segment < split.extra ? 1u : 0u);
		if (!split.dealt && split.num_segments > 1 && segment == split.num_segments - 1u)
			count = split.last;
	}

	__device__ __forceinline__ uint32_t variable_compress_rate(const variable_compress_launch& launch, uint32_t instance, uint32_t segment, uint32_t track, uint32_t kind)
	{
		if (launch.bit_rates == nullptr)
			return (launch.uniform_rates >> (8u * kind)) & 0xFFu;
		return launch.bit_rates[instance * launch.bit_rate_instance_stride + segment * launch.bit_rate_segment_stride + 4ull * track + kind];
	}

	// the x, y, z a sub-track stores of a sample before any range: the rotation normalized and of positive w; translations and scales as registered
	__device__ __forceinline__ float3 variable_compress_value(const f32x4* samples, size_t pose_quads, uint32_t sample, uint32_t track, uint32_t kind)
	{
		const f32x4 v = samples[sample * pose_quads + size_t(track) * 3u + kind];
		if (kind != 0)
			return make_float3(v.x, v.y, v.z);
		const float4 rotation = tracks_compress_positive_w(tracks_compress_normalize(v));
		return make_float3(rotation.x, rotation.y, rotation.z);
	}

	// normalize_sample (normalize.transform.h:200-210): rtm::vector_min keeps its first operand only where it is smaller
	__device__ __forceinline__ float variable_compress_normalize(float value, float range_min, float range_extent)
	{
		const float quotient = (value - range_min) / range_extent;
		const float clamped = quotient < 1.0f ? quotient : 1.0f;
		return range_extent < 0.000000001f ? 0.0f : clamped;
	}
	__device__ __forceinline__ float3 variable_compress_normalize3(float3 v, const float* range)
	{
		return make_float3(variable_compress_normalize(v.x, range[0], range[3]), variable_compress_normalize(v.y, range[1], range[4]), variable_compress_normalize(v.z, range[2], range[5]));
	}

	// pack_scalar_unsigned (math/scalar_packing.h:42-48): scalar_round_symmetric(input * float(2^bits - 1)) of an input in [0, 1]
	__device__ __forceinline__ uint32_t variable_compress_pack(float value, uint32_t bits) { return uint32_t(floorf(value * float((1u << bits) - 1u) + 0.5f)); }

	// fixup_range (normalize.transform.h:133-171) of one component, as written: the padded minimum is the floor of min * 255, or one below
	// it where that is not at or below the minimum; the padded extent the ceil of (max - padded minimum) * 255, or one above it where
	// that does not reach `max` ITSELF (the reference compares the extent with the maximum, not with max - min); both times (1.0F / 255.0F).
	// rtm's min, max and clamp as the selects they are. Returns { padded minimum, padded extent }.
	__device__ __forceinline__ float2 variable_compress_fixup(float range_min, float range_max)
	{
		const float inv_max = 1.0f / 255.0f;
		float quantized_min0 = floorf(range_min * 255.0f);
		quantized_min0 = 0.0f > quantized_min0 ? 0.0f : quantized_min0;
		quantized_min0 = 255.0f < quantized_min0 ? 255.0f : quantized_min0;
		const float below = quantized_min0 - 1.0f;
		const float quantized_min1 = below > 0.0f ? below : 0.0f;
		const float padded_min0 = quantized_min0 * inv_max, padded_min1 = quantized_min1 * inv_max;
		const float padded_min = padded_min0 <= range_min ? padded_min0 : padded_min1;
		float quantized_extent0 = ceilf((range_max - padded_min) * 255.0f);
		quantized_extent0 = 0.0f > quantized_extent0 ? 0.0f : quantized_extent0;
		quantized_extent0 = 255.0f < quantized_extent0 ? 255.0f : quantized_extent0;
		const float above = quantized_extent0 + 1.0f;
		const float quantized_extent1 = above < 255.0f ? above : 255.0f;
		const float padded_extent0 = quantized_extent0 * inv_max, padded_extent1 = quantized_extent1 * inv_max;
		return make_float2(padded_min, padded_extent0 >= range_max ? padded_extent0 : padded_extent1);
	}

	// A segment's range of an animated sub-track: minimum and maximum of its clip-normalized samples [start, start + count), padded by
	// variable_compress_fixup: { padded minimum, padded extent } of x, y and z
	__device__ __forceinline__ void variable_segment_range(const f32x4* samples, size_t pose_quads, uint32_t track, uint32_t kind, const float* clip_range, uint32_t start, uint32_t count, float2 (&padded)[3])
	{
		float low[3] = { 1.0e10f, 1.0e10f, 1.0e10f }, high[3] = { -1.0e10f, -1.0e10f, -1.0e10f };
		for (uint32_t sample = start; sample < start + count; ++sample)
		{
			const float3 v = variable_compress_normalize3(variable_compress_value(samples, pose_quads, sample, track, kind), clip_range);
			const float normalized[3] = { v.x, v.y, v.z };
			#pragma unroll
			for (uint32_t c = 0; c < 3; ++c)
			{
				low[c] = low[c] < normalized[c] ? low[c] : normalized[c];
				high[c] = high[c] > normalized[c] ? high[c] : normalized[c];
			}
		}
		#pragma unroll
		for (uint32_t c = 0; c < 3; ++c)
			padded[c] = variable_compress_fixup(low[c], high[c]);
	}

	// the entry `entry` of an instance's animated sub-tracks in stream order: rotations, translations, scales, each in track order
	struct variable_entry { uint32_t kind, rank, track; };
	__device__ __forceinline__ variable_entry variable_compress_entry(const uint16_t* animated, uint32_t max_tracks, uint32_t num_rotations, uint32_t num_translations, uint32_t entry)
	{
		variable_entry out;
		out.kind = entry < num_rotations ? 0u : entry < num_rotations + num_translations ? 1u : 2u;
		out.rank = entry - (out.kind == 0 ? 0u : out.kind == 1 ? num_rotations : num_rotations + num_translations);
		out.track = animated[out.kind * max_tracks + out.rank];
		return out;
	}

	// where an entry's six segment range bytes begin, from the segment's range data: rotations in groups of four, a row of four per byte
	// (write_range_data.h:243-281: 4 bytes apart); translations and scales six bytes each behind the padded rotations
	__device__ __forceinline__ uint32_t variable_compress_range_at(const variable_entry& entry, uint32_t num_rotations, uint32_t num_translations)
	{
		const uint32_t padded = (num_rotations + 3u) & ~3u;
		return entry.kind == 0 ? entry.rank / 4u * 24u + entry.rank % 4u : 6u * (padded + entry.rank + (entry.kind == 2 ? num_translations : 0u));
	}

	// ---- per (instance, track): the three sub-track types and the clip ranges --------------------------------------------------------------------
	// tracks_compress_analyze_kernel's shape: one wave64 per track, samples across the lanes, over the samples the vote left. Three passes
	// over the samples, each with two shell error ballots (compact.transform.h:72-346): a kind is tested against its sample 0 and against its
	// default under the rotation and translation the passes before it left -- the verdicts are wave uniform behind their ballots. The
	// first pass also takes the minimum and maximum of the nine stored components (normalize.transform.h:51-76). kMetric: the error metric
	// of the six ballots (compress_shell_error, kernels_tracks_compress.inl).
	// kAdditive: both sides of the six shell errors go through A with the sample's base(b, s) (compress_shell_error_on_base).
	template<uint32_t kMetric, bool kAdditive = false>
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void variable_compress_analyze_kernel(variable_compress_launch launch)
	{
		const transform_compress_launch& base = launch.base;
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t track = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		for (uint32_t instance = blockIdx.y; instance < base.num_instances; instance += gridDim.y)
		{
			const compress_instance voted = load_compress_instance(base.instances, instance);
			if (voted.status != 0 || track >= voted.num_tracks)
				continue;
			const uint32_t handle = as_constant(base.raws)[instance];
			const device_raw_tracks raw = load_raw_tracks_fields(base.arrays, handle < base.num_arrays ? handle : 0);
			const float2 shell = base.shells[size_t(instance) * base.max_tracks + track];

			const size_t pose_quads = size_t(raw.num_tracks) * 3u;
			f32x4 default_rotation = { 0.0f, 0.0f, 0.0f, 1.0f }, default_translation = { 0.0f, 0.0f, 0.0f, 0.0f }, default_scale = { 1.0f, 1.0f, 1.0f, 0.0f };
			if (base.default_pose != nullptr)
			{
				default_rotation = base.default_pose[size_t(track) * 3u];
				default_translation = base.default_pose[size_t(track) * 3u + 1u];
				default_scale = base.default_pose[size_t(track) * 3u + 2u];
			}
			const qvv first = tracks_compress_sample(raw.samples, pose_quads, 0, track);
			const float4 rotation0 = tracks_compress_positive_w(first.rotation);
			[[maybe_unused]] compress_additive_base additive = {};
			if constexpr (kAdditive)
				additive = compress_additive_base_of(base, instance, raw);
			// the base sample that goes with a sample of the clip (read anew in every pass: nothing of the base is kept)
			const auto base_of = [&](uint32_t sample) __attribute__((always_inline)) -> qvv
			{
				if constexpr (kAdditive)
					return compress_base_sample(additive, track, compress_base_key(additive, sample));
				else
					return qvv{};
			};

			// the rotation, as in tracks_compress_analyze_kernel, and the ranges
			float low[9], high[9];
			#pragma unroll
			for (uint32_t c = 0; c < 9; ++c)
			{
				low[c] = 1.0e10f;
				high[c] = -1.0e10f;
			}
			bool moves = false, leaves_default = false;
			for (uint32_t sample = lane; sample < voted.num_out_samples; sample += k_wave_size)
			{
				qvv kept = tracks_compress_sample(raw.samples, pose_quads, sample, track);
				kept.rotation = tracks_compress_positive_w(kept.rotation);
				qvv other = kept;
				other.rotation = rotation0;
				[[maybe_unused]] const qvv base_transform = base_of(sample);
				moves = moves || compress_shell_error_on_base<kMetric, kAdditive>(shell.x, additive, base_transform, kept, other) > shell.y;
				other.rotation = make_float4(default_rotation.x, default_rotation.y, default_rotation.z, default_rotation.w);
				leaves_default = leaves_default || compress_shell_error_on_base<kMetric, kAdditive>(shell.x, additive, base_transform, kept, other) > shell.y;
				const float stored[9] = { kept.rotation.x, kept.rotation.y, kept.rotation.z, kept.translation.x, kept.translation.y, kept.translation.z, kept.scale.x, kept.scale.y, kept.scale.z };
				#pragma unroll
				for (uint32_t c = 0; c < 9; ++c)
				{
					low[c] = low[c] < stored[c] ? low[c] : stored[c];
					high[c] = high[c] > stored[c] ? high[c] : stored[c];
				}
			}
			const uint32_t rotation_type = transform_compress_type(__ballot(moves) == 0, __ballot(leaves_default) == 0);

			// the translation under the rotation as it was compacted: r_0 of a constant one, the default rotation as given
			const float4 constant_rotation = rotation_type == k_sub_track_constant ? rotation0 : make_float4(default_rotation.x, default_rotation.y, default_rotation.z, default_rotation.w);
			moves = leaves_default = false;
			for (uint32_t sample = lane; sample < voted.num_out_samples; sample += k_wave_size)
			{
				qvv kept = tracks_compress_sample(raw.samples, pose_quads, sample, track);
				kept.rotation = rotation_type == k_sub_track_animated ? tracks_compress_positive_w(kept.rotation) : constant_rotation;
				qvv other = kept;
				other.translation = first.translation;
				[[maybe_unused]] const qvv base_transform = base_of(sample);
				moves = moves || compress_shell_error_on_base<kMetric, kAdditive>(shell.x, additive, base_transform, kept, other) > shell.y;
				other.translation = make_float4(default_translation.x, default_translation.y, default_translation.z, 0.0f);
				leaves_default = leaves_default || compress_shell_error_on_base<kMetric, kAdditive>(shell.x, additive, base_transform, kept, other) > shell.y;
			}
			const uint32_t translation_type = transform_compress_type(__ballot(moves) == 0, __ballot(leaves_default) == 0);

			// the scale under both
			const float4 constant_translation = translation_type == k_sub_track_constant ? first.translation : make_float4(default_translation.x, default_translation.y, default_translation.z, 0.0f);
			moves = leaves_default = false;
			for (uint32_t sample = lane; sample < voted.num_out_samples; sample += k_wave_size)
			{
				qvv kept = tracks_compress_sample(raw.samples, pose_quads, sample, track);
				kept.rotation = rotation_type == k_sub_track_animated ? tracks_compress_positive_w(kept.rotation) : constant_rotation;
				if (translation_type != k_sub_track_animated)
					kept.translation = constant_translation;
				qvv other = kept;
				other.scale = first.scale;
				[[maybe_unused]] const qvv base_transform = base_of(sample);
				moves = moves || compress_shell_error_on_base<kMetric, kAdditive>(shell.x, additive, base_transform, kept, other) > shell.y;
				other.scale = make_float4(default_scale.x, default_scale.y, default_scale.z, 0.0f);
				leaves_default = leaves_default || compress_shell_error_on_base<kMetric, kAdditive>(shell.x, additive, base_transform, kept, other) > shell.y;
			}
			const uint32_t scale_type = transform_compress_type(__ballot(moves) == 0, __ballot(leaves_default) == 0);

			// the ranges over the wave: a butterfly; of two zeros the reference keeps the later sample's (rtm::vector_min and vector_max
			// return their second operand when the two compare equal): found again in a pass of its own, which real data never takes
			#pragma unroll
			for (uint32_t c = 0; c < 9; ++c)
			{
				#pragma unroll
				for (int offset = int(k_wave_size) / 2; offset != 0; offset >>= 1)
				{
					const float other_low = __shfl_xor(low[c], offset), other_high = __shfl_xor(high[c], offset);
					low[c] = other_low < low[c] ? other_low : low[c];
					high[c] = other_high > high[c] ? other_high : high[c];
				}
				if (low[c] == 0.0f || high[c] == 0.0f)
				{
					uint32_t last_zero = 0;			// (sample + 1) << 1 | sign bit of the last zero sample of this lane
					for (uint32_t sample = lane; sample < voted.num_out_samples; sample += k_wave_size)
					{
						const float3 v = variable_compress_value(raw.samples, pose_quads, sample, track, c / 3u);
						const float value = c % 3u == 0 ? v.x : c % 3u == 1 ? v.y : v.z;
						if (value == 0.0f)
							last_zero = ((sample + 1u) << 1) | (__float_as_uint(value) >> 31);
					}
					#pragma unroll
					for (int offset = int(k_wave_size) / 2; offset != 0; offset >>= 1)
					{
						const uint32_t other = uint32_t(__shfl_xor(int(last_zero), offset));
						last_zero = other > last_zero ? other : last_zero;
					}
					const float zero = __uint_as_float(last_zero << 31);
					low[c] = low[c] == 0.0f ? zero : low[c];
					high[c] = high[c] == 0.0f ? zero : high[c];
				}
			}
			if (lane == 0)
			{
				base.track_flags[size_t(instance) * base.max_tracks + track] = uint8_t(rotation_type | (translation_type << 2) | (scale_type << 4));
				float* ranges = launch.clip_ranges + (size_t(instance) * base.max_tracks + track) * k_variable_range_floats;
				#pragma unroll
				for (uint32_t kind = 0; kind < 3; ++kind)
				{
					#pragma unroll
					for (uint32_t c = 0; c < 3; ++c)
					{
						ranges[kind * 6u + c] = low[kind * 3u + c];
						ranges[kind * 6u + 3u + c] = high[kind * 3u + c] - low[kind * 3u + c];
					}
				}
			}
		}
	}

	// the sum of a value over the lanes up to and including this one
	__device__ __forceinline__ uint32_t variable_compress_scan(uint32_t value, uint32_t lane)
	{
		#pragma unroll
		for (uint32_t offset = 1; offset < k_wave_size; offset <<= 1)
		{
			const uint32_t other = uint32_t(__shfl_up(int(value), offset));
			value += lane >= offset ? other : 0u;
		}
		return value;
	}

	// ---- per instance: the segments, the prefix sums, the refusals, and everything but segment ranges and streams ------------------------------
	// One wave64 per instance, as transform_compress_layout_kernel, whose refusal, common header words, constant rotations and metadata
	// these are. In front of any write to the row: the counts and the lists of animated tracks (lanes <-> tracks), then per segment the bit widths of the animated sub-tracks in stream order (lanes <-> entries of the
	// lists), their prefix sums and where the segment's three parts lie -- all into the workspace --, and with the last segment the size:
	// the refusals. Then the row: headers, start indices, segment headers (compress.transform.impl.h:404-470, write_segment_data.h:67-122),
	// types, constants (write_stream_data.h:199-310), clip range data (write_range_data.h:60-207), per segment the format bytes
	// (write_stream_data.h:460-531) and every padding byte, the metadata or the tail.
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void variable_compress_layout_kernel(variable_compress_launch launch)
	{
		const transform_compress_launch& base = launch.base;
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t instance = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		if (instance >= base.num_instances)
			return;

		const uint32_t handle = as_constant(base.raws)[instance];
		const device_raw_tracks raw = load_raw_tracks_fields(base.arrays, handle < base.num_arrays ? handle : 0);
		const uint32_t num_tracks = raw.num_tracks;
		const uint8_t* track_flags = base.track_flags + size_t(instance) * base.max_tracks;
		uint16_t* animated = base.animated + size_t(instance) * 3u * base.max_tracks;

		compress_instance record = {};
		const compress_instance voted = load_compress_instance(base.instances, instance);
		uint32_t status = voted.status;
		const uint32_t num_samples = voted.num_out_samples;
		if (status == 0 && num_samples > launch.max_samples)
			status = k_compress_status_refused;

		// the counts and the lists
		uint32_t num_constant[3] = { 0, 0, 0 }, num_animated[3] = { 0, 0, 0 };
		if (status == 0)
		{
			for (uint32_t first = 0; first < num_tracks; first += k_wave_size)
			{
				const uint32_t track = first + lane;
				const uint32_t flags = track < num_tracks ? track_flags[track] : 0u;
				#pragma unroll
				for (uint32_t kind = 0; kind < 3; ++kind)
				{
					const uint32_t type = (flags >> (2u * kind)) & 3u;
					const uint64_t animated_mask = __ballot(type == k_sub_track_animated);
					if (type == k_sub_track_animated)
						animated[kind * base.max_tracks + num_animated[kind] + transform_compress_rank(animated_mask)] = uint16_t(track);
					num_constant[kind] += uint32_t(__popcll(__ballot(type == k_sub_track_constant)));
					num_animated[kind] += uint32_t(__popcll(animated_mask));
				}
			}
			__threadfence();		// (the lists are read back below by other lanes of this wave)
		}

		const bool has_scale = num_constant[2] + num_animated[2] != 0;
		const bool with_descriptions = (base.flags & k_compress_include_descriptions) != 0;
		const bool with_parents = with_descriptions || (base.flags & k_compress_include_parents) != 0;
		const uint32_t num_entries = num_animated[0] + num_animated[1] + num_animated[2];
		const uint32_t padded_rotations = (num_animated[0] + 3u) & ~3u;
		const uint32_t num_variable = padded_rotations + num_animated[1] + num_animated[2];
		const variable_split split = variable_split_of(num_samples);
		const uint32_t num_segments = split.num_segments;
		const bool multiple = num_segments > 1;
		const uint32_t type_words = (num_tracks + 15u) / 16u;
		const uint32_t start_indices_at = k_transform_header_offset + k_segment_start_indices_offset;
		const uint64_t segment_headers_at = start_indices_at + (multiple ? 4ull * (uint64_t(num_segments) + 1u) : 0ull);
		const uint64_t types_at = segment_headers_at + 16ull * num_segments;
		const uint64_t constants_at = types_at + 4ull * type_words * (has_scale ? 3u : 2u);
		const uint64_t clip_ranges_at = constants_at + 12ull * (num_constant[0] + num_constant[1] + num_constant[2]);
		uint64_t cursor = clip_ranges_at + 24ull * num_entries;

		// per segment: the widths, their prefix sums, the three parts
		variable_segment* segments = launch.segments + size_t(instance) * launch.max_segments;
		bool bad_rate = false;
		for (uint32_t segment = 0; status == 0 && segment < num_segments; ++segment)
		{
			uint32_t* prefix = launch.prefix + (size_t(instance) * launch.max_segments + segment) * 3u * base.max_tracks;
			uint32_t pose_bits = 0;
			for (uint32_t first = 0; first < num_entries; first += k_wave_size)
			{
				uint32_t width = 0;
				if (first + lane < num_entries)
				{
					const variable_entry entry = variable_compress_entry(animated, base.max_tracks, num_animated[0], num_animated[1], first + lane);
					const uint32_t rate = variable_compress_rate(launch, instance, segment, entry.track, entry.kind);
					bad_rate = bad_rate || rate > k_variable_raw_rate || (rate == 0 && !multiple);
					width = rate > k_variable_raw_rate ? 0u : rate == k_variable_raw_rate ? 96u : 3u * rate;
				}
				const uint32_t through = variable_compress_scan(width, lane);
				if (first + lane < num_entries)
					prefix[first + lane] = pose_bits + through - width;
				pose_bits += uint32_t(__shfl(int(through), int(k_wave_size) - 1));
			}
			variable_segment out;
			variable_segment_samples(split, segment, out.start, out.count);
			out.pose_bits = pose_bits;
			const uint64_t formats_at = cursor;
			const uint64_t ranges_at = (formats_at + num_variable + 1u) & ~1ull;
			const uint64_t stream_at = (ranges_at + (multiple ? 6ull * num_variable : 0ull) + 3u) & ~3ull;
			const uint64_t stream_bytes = (uint64_t(pose_bits) * out.count + 7u) / 8u;
			cursor = stream_at + stream_bytes;
			// (the reference counts a segment's bits and every offset in 32 bits)
			if (cursor > 0xFFFFFFFFull || uint64_t(pose_bits) * out.count > 0xFFFFFFFFull)
				status = k_compress_status_refused;
			out.stream_bytes = uint32_t(stream_bytes);
			out.formats_at = uint32_t(formats_at);
			out.ranges_at = uint32_t(ranges_at);
			out.stream_at = uint32_t(stream_at);
			out.unused = 0;
			if (lane == 0)
				segments[segment] = out;
		}
		if (__ballot(bad_rate) != 0)
			status |= k_compress_status_refused;
		__threadfence();			// (the segments are read back below by every lane)

		const uint64_t metadata_at = with_parents ? (cursor + 3u) & ~3ull : cursor;
		const uint64_t size = metadata_at + (with_parents ? 4ull * num_tracks + (with_descriptions ? 48ull * num_tracks : 0ull) + sizeof(optional_metadata_header) : 15ull);
		if (status == 0 && (size > base.blob_stride_bytes || size > 0xFFFFFFFFull))
			status = k_compress_status_refused;

		if (status != 0)
		{
			if (lane == 0)
			{
				record.status = status;
				base.instances[instance] = record;
				compress_write_refusal(base, instance, status);
			}
			return;
		}

		uint8_t* blob = base.blobs + uint64_t(instance) * base.blob_stride_bytes;
		uint32_t* words = reinterpret_cast<uint32_t*>(blob);
		if (lane == 0)
		{
			record.samples = reinterpret_cast<const float*>(raw.samples);
			record.num_tracks = num_tracks;
			record.num_samples = voted.num_samples;
			record.num_out_samples = num_samples;
			record.num_components = num_segments;		// (a transform array has no component count: this call keeps its segment count here)
			record.track_type = k_track_type_qvvf;
			record.wrap = voted.wrap;
			record.sample_rate = raw.sample_rate;
			record.size = uint32_t(size);
			record.num_animated = num_animated[0];
			record.num_animated_translations = num_animated[1];
			record.num_animated_scales = num_animated[2];
			base.instances[instance] = record;
			base.results[instance] = make_uint2(ACLHIP_COMPRESS_OK, uint32_t(size));

			transform_compress_write_common_header(words, uint32_t(size), num_tracks, num_samples, raw.sample_rate, num_animated, num_constant);
			// has_scale | default scale 1 (0 for an additive1 clip) | vector3f_variable twice | quatf_drop_w_variable | no database, no trivial defaults, no stripped
			// key frames | wrap optimized | metadata
			words[7] = (has_scale ? 1u : 0u) | transform_compress_default_scale_bit(base) | (uint32_t(k_vector_vector3f_variable) << 2) | (uint32_t(k_vector_vector3f_variable) << 3)
				| (uint32_t(k_rotation_quatf_drop_w_variable) << 4) | (voted.wrap != 0 ? 1u << 30 : 0u) | (with_parents ? 1u << 31 : 0u);
			words[8] = num_segments;					// transform_tracks_header; offsets from its own start
			words[9] = num_variable;
			words[17] = uint32_t(segment_headers_at) - k_transform_header_offset;
			words[18] = uint32_t(types_at) - k_transform_header_offset;
			words[19] = uint32_t(constants_at) - k_transform_header_offset;
			words[20] = uint32_t(clip_ranges_at) - k_transform_header_offset;
			if (multiple)
				words[start_indices_at / 4u + num_segments] = 0xFFFFFFFFu;
		}

		// start indices, segment headers, format bytes and the padding of every segment
		for (uint32_t segment = 0; segment < num_segments; ++segment)
		{
			const variable_segment at = segments[segment];
			const uint32_t* prefix = launch.prefix + (size_t(instance) * launch.max_segments + segment) * 3u * base.max_tracks;
			if (lane == 0)
			{
				if (multiple)
					words[start_indices_at / 4u + segment] = at.start;
				uint32_t* header = words + segment_headers_at / 4u + 4u * segment;
				header[0] = at.pose_bits;
				header[1] = num_animated[0] < num_entries ? prefix[num_animated[0]] : at.pose_bits;
				header[2] = (num_animated[0] + num_animated[1] < num_entries ? prefix[num_animated[0] + num_animated[1]] : at.pose_bits) - header[1];
				header[3] = at.formats_at - k_transform_header_offset;
			}
			for (uint32_t first = 0; first < num_entries; first += k_wave_size)
			{
				if (first + lane >= num_entries)
					continue;
				const variable_entry entry = variable_compress_entry(animated, base.max_tracks, num_animated[0], num_animated[1], first + lane);
				const uint32_t rate = variable_compress_rate(launch, instance, segment, entry.track, entry.kind);
				blob[at.formats_at + first + lane + (entry.kind != 0 ? padded_rotations - num_animated[0] : 0u)] = uint8_t(rate == k_variable_raw_rate ? k_variable_raw_format : rate);
			}
			// the padding: the formats and (with segment ranges) the range rows of a last partial group of rotations, one byte in front of
			// the range data, up to three in front of the stream
			if (lane < padded_rotations - num_animated[0])
			{
				const uint32_t rank = num_animated[0] + lane;
				blob[at.formats_at + rank] = 0;
				if (multiple)
					for (uint32_t row = 0; row < 6; ++row)
						blob[at.ranges_at + rank / 4u * 24u + rank % 4u + 4u * row] = 0;
			}
			const uint32_t formats_end = at.formats_at + num_variable, ranges_end = at.ranges_at + (multiple ? 6u * num_variable : 0u);
			if (lane < at.ranges_at - formats_end)
				blob[formats_end + lane] = 0;
			if (lane < at.stream_at - ranges_end)
				blob[ranges_end + lane] = 0;
		}

		// every track's type and constant sample
		const uint32_t* first_frame = reinterpret_cast<const uint32_t*>(raw.samples);
		uint32_t constants_before[3] = { 0, 0, 0 };
		const uint32_t section_at[3] = { uint32_t(constants_at), uint32_t(constants_at) + 12u * num_constant[0], uint32_t(constants_at) + 12u * (num_constant[0] + num_constant[1]) };
		for (uint32_t first = 0; first < num_tracks; first += k_wave_size)
		{
			const uint32_t track = first + lane;
			const uint32_t flags = track < num_tracks ? track_flags[track] : 0u;
			#pragma unroll
			for (uint32_t kind = 0; kind < 3; ++kind)
			{
				const uint32_t type = (flags >> (2u * kind)) & 3u;
				const uint64_t constant_mask = __ballot(type == k_sub_track_constant);
				if (type == k_sub_track_constant)
				{
					const uint32_t rank = constants_before[kind] + transform_compress_rank(constant_mask);
					const uint32_t* in = first_frame + size_t(track) * 12u + kind * 4u;
					if (kind == 0)
						transform_compress_write_constant_rotation(reinterpret_cast<uint32_t*>(blob + section_at[0]), in, rank, num_constant[0]);
					else
					{
						uint32_t* out = reinterpret_cast<uint32_t*>(blob + section_at[kind]) + rank * 3u;
						out[0] = in[0];
						out[1] = in[1];
						out[2] = in[2];
					}
				}
				constants_before[kind] += uint32_t(__popcll(constant_mask));
				const uint32_t packed = transform_compress_pack_types(type, lane);
				if ((kind < 2 || has_scale) && (lane & 15u) == 0 && track < num_tracks)
					reinterpret_cast<uint32_t*>(blob + types_at)[kind * type_words + track / 16u] = packed;
			}
		}

		// clip range data: rotations in groups of four as min xxxx yyyy zzzz, extent xxxx yyyy zzzz (a last group of n: rows of n);
		// translations, then scales, as min xyz extent xyz
		for (uint32_t first = 0; first < num_entries; first += k_wave_size)
		{
			if (first + lane >= num_entries)
				continue;
			const variable_entry entry = variable_compress_entry(animated, base.max_tracks, num_animated[0], num_animated[1], first + lane);
			const uint32_t* range = reinterpret_cast<const uint32_t*>(launch.clip_ranges + (size_t(instance) * base.max_tracks + entry.track) * k_variable_range_floats + entry.kind * 6u);
			uint32_t* out = reinterpret_cast<uint32_t*>(blob + clip_ranges_at);
			if (entry.kind == 0)
			{
				const uint32_t group = entry.rank / 4u, place = entry.rank % 4u, group_size = num_animated[0] - group * 4u < 4u ? num_animated[0] - group * 4u : 4u;
				for (uint32_t row = 0; row < 6; ++row)
					out[group * 24u + row * group_size + place] = range[row];
			}
			else
				for (uint32_t row = 0; row < 6; ++row)
					out[(first + lane) * 6u + row] = range[row];
		}

		if (!with_parents)
		{
			// 15 zero bytes behind a stream that ends on any byte; nothing behind `size` is touched
			if (lane < 15)
				blob[cursor + lane] = 0;
			return;
		}
		if (lane < metadata_at - cursor)
			blob[cursor + lane] = 0;

		transform_compress_write_tail(base, blob, metadata_at, num_tracks, lane, with_descriptions);
	}

	// ---- per (instance, segment): the segment ranges ---------------------------------------------------------------------------------------------
	// One wave64 per (instance, segment) of a blob with more than one segment, lanes <-> animated sub-tracks in stream order: a lane walks
	// the segment's samples (31 at most) of its sub-track, clip-normalizes each, keeps minimum and maximum, applies fixup_range
	// (normalize.transform.h:133-171, as written) and stores the six range bytes -- or, at rate 0, the segment's first clip-normalized
	// sample on 3 x 16 bits (quantize.transform.h:383-394, segment.transform.h:242-244) in the same six bytes. The padded rows of a last
	// partial group of rotations are the layout's.
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void variable_compress_ranges_kernel(variable_compress_launch launch)
	{
		const transform_compress_launch& base = launch.base;
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint64_t num_waves = uint64_t(base.num_instances) * launch.max_segments;
		for (uint64_t wave = uint64_t(blockIdx.x) * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size); wave < num_waves;
			wave += uint64_t(gridDim.x) * k_compress_waves_per_block)
		{
			const uint32_t instance = uint32_t(wave / launch.max_segments), segment = uint32_t(wave % launch.max_segments);
			const compress_instance record = load_compress_instance(base.instances, instance);
			if (record.status != 0 || record.num_components < 2 || segment >= record.num_components)
				continue;
			const variable_segment at = launch.segments[size_t(instance) * launch.max_segments + segment];
			const uint16_t* animated = base.animated + size_t(instance) * 3u * base.max_tracks;
			const f32x4* samples = reinterpret_cast<const f32x4*>(record.samples);
			const size_t pose_quads = size_t(record.num_tracks) * 3u;
			uint8_t* ranges = base.blobs + uint64_t(instance) * base.blob_stride_bytes + at.ranges_at;
			const uint32_t num_entries = record.num_animated + record.num_animated_translations + record.num_animated_scales;
			for (uint32_t index = lane; index < num_entries; index += k_wave_size)
			{
				const variable_entry entry = variable_compress_entry(animated, base.max_tracks, record.num_animated, record.num_animated_translations, index);
				const float* clip_range = launch.clip_ranges + (size_t(instance) * base.max_tracks + entry.track) * k_variable_range_floats + entry.kind * 6u;
				const uint32_t rate = variable_compress_rate(launch, instance, segment, entry.track, entry.kind);
				uint8_t* out = ranges + variable_compress_range_at(entry, record.num_animated, record.num_animated_translations);
				const uint32_t step = entry.kind == 0 ? 4u : 1u;
				if (rate == 0)
				{
					const float3 v = variable_compress_normalize3(variable_compress_value(samples, pose_quads, at.start, entry.track, entry.kind), clip_range);
					const uint32_t x = variable_compress_pack(v.x, 16), y = variable_compress_pack(v.y, 16), z = variable_compress_pack(v.z, 16);
					// a rotation's rows take the high byte first (write_range_data.h:248-258); a vector is three little endian u16
					const uint32_t high_first = entry.kind == 0 ? 8u : 0u;
					out[0] = uint8_t(x >> high_first);
					out[step] = uint8_t(x >> (8u - high_first));
					out[2u * step] = uint8_t(y >> high_first);
					out[3u * step] = uint8_t(y >> (8u - high_first));
					out[4u * step] = uint8_t(z >> high_first);
					out[5u * step] = uint8_t(z >> (8u - high_first));
					continue;
				}
				float2 padded[3];
				variable_segment_range(samples, pose_quads, entry.track, entry.kind, clip_range, at.start, at.count, padded);
				#pragma unroll
				for (uint32_t c = 0; c < 3; ++c)
				{
					out[c * step] = uint8_t(variable_compress_pack(padded[c].x, 8));
					out[(3u + c) * step] = uint8_t(variable_compress_pack(padded[c].y, 8));
				}
			}
		}
	}

	// ---- the bit streams ----------------------------------------------------------------------------------------------------------------------
	// The property of transform_compress_stream_kernel kept: a lane owns one DWORD of a segment's animated stream (write_stream_data.h:312-458:
	// samples ascending, per sample rotations, translations, scales in track order, sub-tracks of rate 0 absent, every field most significant
	// bit first, continuous across samples, rounded up to a byte once per segment). A division by the pose's bits gives the sample, a binary
	// search of the segment's prefix sums the last sub-track that begins at or in front of the dword's first bit -- the one that reaches
	// into it: a sub-track without bits shares its offset with the next --, and the lane walks forward from there, recomputing every
	// component from the registered sample, the clip range (the workspace) and the segment range (the six bytes the launch before stored:
	// byte * (1.0F / 255.0F) is the padded value fixup_range made), until its 32 bits are full or the segment ends. One byte swapped,
	// coalesced store; the last dword of a segment may end inside the next segment's format bytes and goes byte by byte.
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void variable_compress_stream_kernel(variable_compress_launch launch)
	{
		const transform_compress_launch& base = launch.base;
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t wave = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		const uint32_t instance = wave / base.waves_per_instance;
		const uint32_t share = wave - instance * base.waves_per_instance;
		if (instance >= base.num_instances)
			return;

		const compress_instance record = load_compress_instance(base.instances, instance);
		if (record.status != 0)
			return;
		const uint32_t num_entries = record.num_animated + record.num_animated_translations + record.num_animated_scales;
		if (num_entries == 0)
			return;
		const bool multiple = record.num_components > 1;
		const uint16_t* animated = base.animated + size_t(instance) * 3u * base.max_tracks;
		const f32x4* samples = reinterpret_cast<const f32x4*>(record.samples);
		const size_t pose_quads = size_t(record.num_tracks) * 3u;
		uint8_t* blob = base.blobs + uint64_t(instance) * base.blob_stride_bytes;

		for (uint32_t segment = 0; segment < record.num_components; ++segment)
		{
			const variable_segment at = launch.segments[size_t(instance) * launch.max_segments + segment];
			const uint32_t* prefix = launch.prefix + (size_t(instance) * launch.max_segments + segment) * 3u * base.max_tracks;
			const uint32_t num_dwords = (at.stream_bytes + 3u) / 4u;
			for (uint32_t dword = share * k_wave_size + lane; dword < num_dwords; dword += base.waves_per_instance * k_wave_size)
			{
				const uint64_t first_bit = 32ull * dword;
				uint32_t sample = uint32_t(first_bit / at.pose_bits);
				const uint32_t in_pose = uint32_t(first_bit - uint64_t(sample) * at.pose_bits);
				uint32_t low = 0, high = num_entries - 1u;
				while (low < high)
				{
					const uint32_t middle = (low + high + 1u) / 2u;
					if (prefix[middle] <= in_pose)
						low = middle;
					else
						high = middle - 1u;
				}
				uint32_t index = low, in_entry = in_pose - prefix[low];
				uint32_t word = 0, need = 32;
				while (need != 0 && sample < at.count)
				{
					const uint32_t begin = prefix[index], end = index + 1u < num_entries ? prefix[index + 1u] : at.pose_bits;
					const uint32_t bits = (end - begin) / 3u;
					if (bits != 0)
					{
						const variable_entry entry = variable_compress_entry(animated, base.max_tracks, record.num_animated, record.num_animated_translations, index);
						float3 v = variable_compress_value(samples, pose_quads, at.start + sample, entry.track, entry.kind);
						uint32_t quantized[3] = { __float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z) };
						if (bits != 32)
						{
							v = variable_compress_normalize3(v, launch.clip_ranges + (size_t(instance) * base.max_tracks + entry.track) * k_variable_range_floats + entry.kind * 6u);
							if (multiple)
							{
								const uint8_t* range = blob + at.ranges_at + variable_compress_range_at(entry, record.num_animated, record.num_animated_translations);
								const uint32_t step = entry.kind == 0 ? 4u : 1u;
								const float segment_range[6] = { float(range[0]) * (1.0f / 255.0f), float(range[step]) * (1.0f / 255.0f), float(range[2u * step]) * (1.0f / 255.0f),
									float(range[3u * step]) * (1.0f / 255.0f), float(range[4u * step]) * (1.0f / 255.0f), float(range[5u * step]) * (1.0f / 255.0f) };
								v = variable_compress_normalize3(v, segment_range);
							}
							quantized[0] = variable_compress_pack(v.x, bits);
							quantized[1] = variable_compress_pack(v.y, bits);
							quantized[2] = variable_compress_pack(v.z, bits);
						}
						uint32_t component = in_entry / bits, used = in_entry - component * bits;
						while (need != 0 && component < 3)
						{
							const uint32_t value = component == 0 ? quantized[0] : component == 1 ? quantized[1] : quantized[2];
							const uint32_t left = bits - used, take = left < need ? left : need;
							const uint32_t piece = take == 32 ? value : (value >> (left - take)) & ((1u << take) - 1u);
							word = take == 32 ? piece : (word << take) | piece;
							need -= take;
							used += take;
							if (used == bits)
							{
								used = 0;
								++component;
							}
						}
					}
					in_entry = 0;
					if (++index == num_entries)
					{
						index = 0;
						++sample;
					}
				}
				word = need < 32 ? word << need : 0u;
				if (4u * dword + 4u <= at.stream_bytes)
					reinterpret_cast<uint32_t*>(blob + at.stream_at)[dword] = __builtin_bswap32(word);
				else
					for (uint32_t byte = 4u * dword; byte < at.stream_bytes; ++byte)
						blob[at.stream_at + byte] = uint8_t(word >> (24u - 8u * (byte - 4u * dword)));
			}
		}
	}
