// kernels_pose_buffers.inl -- part of aclhip.hip (one translation unit; included there behind kernels_skeleton.inl, not compiled on its own).
// The pose consumers over a CALLER'S pose buffers (aclhip_transform_poses_batch): transform_poses_kernel fills its LDS image from a row
// in HBM instead of from a clip, and everything behind the fill is decompress_poses_consumer_kernel's finish_consumer_poses with the
// skeleton's bone count and walk schedule -- the combine with a base buffer, the walk, the store and the bounds.
// inverse_transform_poses_kernel (aclhip_inverse_transform_poses_batch) is the way back over the same rows: object -> local space and
// make-additive, a bone per lane, no walk.
// measure_pose_error_kernel (aclhip_measure_pose_error_batch) holds TWO rows per instance, takes both through the same additive step and the
// same walk without storing them, and measures per bone how far three points on the bone's shell moved.
// pose_matrices_kernel (aclhip_pose_matrices_batch) writes 3x4 matrices, local or object space, with the matrix walk of the reference's
// qvvf_matrix3x4f_transform_error_metric; measure_pose_error_kernel's kMatrices instantiations are the measure in that arithmetic.
// skinning_matrices_kernel (aclhip_skinning_matrices_batch) is pose_matrices_kernel with a palette for its store: one body, two writers.
// What the six kernels do alike stands first, once: the two ends of their arguments, the opening of an instance with the refusal every
// launch shares (open_instance, count_refused), the fill of an image from a row (fill_image_from_row), the closing of a walk slot
// without work (close_idle_walk_slot).

	// ---- what the kernels over a caller's pose rows do alike ------------------------------------------------------------------------------
	// The two ends of every kernel's argument (the host fills them: pose_rows_head_of, pose_rows_shape_of). Two records, not one: the
	// skeletons stay the first 24 bytes of the argument and the shape stays behind the launch's own rows, so the rows between them keep
	// their places among the argument words that arrive preloaded in SGPRs. Kernels and helpers take them BY VALUE: read through a
	// reference, an argument word is loaded again behind every atomic (the blend's object space kernels paid two VGPRs for it).
	struct pose_rows_head
	{
		const device_skeleton* skeletons;		// the context's skeleton table
		uint32_t num_skeletons;					// its capacity
		uint32_t skeleton;						// the launch's skeleton, when instance_skeletons is null
		const uint32_t* instance_skeletons;		// [num_instances] or null
	};
	struct pose_rows_shape
	{
		uint32_t num_instances;
		uint32_t lds_quads_per_image, lds_bytes_per_instance;		// as decompress_poses_consumer_kernel takes them
		uint32_t packed_block_shape;			// log2 of the instances per workgroup (bits 0..7) | words of LDS reserved for the shared walk schedule (bits 8..31)
		unsigned long long* rejected_count;
		__device__ __forceinline__ uint32_t log2_instances_per_block() const { return packed_block_shape & 0xFFu; }
		__device__ __forceinline__ uint32_t schedule_words() const { return packed_block_shape >> 8; }
	};

	// An instance of a launch, opened: its skeleton's record with every field on the scalar unit, and what every launch refuses of it.
	// Record 0 is never handed out and a cleared record (reference_pose == null) is an unknown or retired skeleton; kNeedsHierarchy: the
	// launch walks or reads parents, and the skeleton has no hierarchy; more bones than the launch's LDS image holds (the image is sized
	// from a stride on the host, and a skeleton may be registered behind a captured launch's back). Wave uniform, and in front of any load
	// of a row: a kernel ORs in its own clauses -- its strides, its masks, its skin, its tables -- and serves what is left, which then
	// reads and writes inside its own rows.
	struct opened_instance { device_skeleton skeleton; uint32_t num_bones; bool refused; };
	template<bool kNeedsHierarchy>
	__device__ __forceinline__ opened_instance open_instance(pose_rows_head head, pose_rows_shape shape, uint32_t instance)
	{
		const uint32_t skeleton_id = head.instance_skeletons != nullptr ? as_constant(head.instance_skeletons)[instance] : head.skeleton;
		const device_skeleton skeleton = load_skeleton_fields(head.skeletons, skeleton_id < head.num_skeletons ? skeleton_id : 0);
		const bool refused = skeleton_id >= head.num_skeletons || skeleton.reference_pose == nullptr || (kNeedsHierarchy && skeleton.hierarchy == nullptr)
			|| skeleton.num_bones * 3u > shape.lds_quads_per_image;
		return opened_instance{ skeleton, skeleton.num_bones, refused };
	}

	// a refused instance is counted once, by the wave that opened it (aclhip_get_rejected_instance_count)
	__device__ __forceinline__ void count_refused(unsigned long long* rejected_count, uint32_t lane)
	{
		if (lane == 0)
			atomicAdd(rejected_count, 1ull);
	}

	// A row straight into an LDS image by DMA, lanes <-> consecutive quads (the LDS side of a piece is wave uniform + lane * 16). Nothing
	// waits here: the caller's next wave_lds_barrier does (vmcnt), in front of the first LDS read.
	__device__ __forceinline__ void fill_image_from_row(f32x4* image, const uint8_t* row, uint32_t num_quads, uint32_t lane)
	{
		const f32x4* source = reinterpret_cast<const f32x4*>(row);
		for (uint32_t base = 0; base < num_quads; base += k_wave_size)
		{
			if (base + lane < num_quads)
				__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(source + base + lane),
					(__attribute__((address_space(3))) void*)(image + base), 16, 0, 0);
		}
	}

	// A slot without work clears its entry of the walk (a slot with work has its steps and its schedule already: request_walk_schedule).
	// Called by the one lane that speaks for the slot.
	__device__ __forceinline__ void close_idle_walk_slot(consumer_walk_slots& walk, uint32_t slot, uint32_t num_bones)
	{
		if (num_bones == 0)
		{
			walk.levels[slot] = 0;
			walk.schedules[slot] = nullptr;
		}
	}

	// ---- object space and additive apply (aclhip_transform_poses_batch) -------------------------------------------------------------------
	// the kernel's argument: the launch's three buffers between the two shared ends
	struct pose_buffer_launch
	{
		pose_rows_head head;
		const uint8_t* local_poses;				// row i at local_poses + i * local_pose_stride_bytes
		uint64_t local_pose_stride_bytes;
		const uint8_t* additive_poses;			// kBase == k_consumer_base_buffer: row i at additive_poses + i * additive_pose_stride_bytes
		uint64_t additive_pose_stride_bytes;
		uint8_t* poses;							// null: the boxes alone (bounds instantiations)
		uint64_t pose_stride_bytes;
		uint32_t additive_format;
		pose_rows_shape shape;
	};

	// One wave64 per instance, up to 8 instances per workgroup, images as consumer_wave_of lays them out.
	//   kObjectSpace   local_to_object_space with the skeleton's walk schedule
	//   kBase          k_consumer_base_none: the image is the local row L. k_consumer_base_buffer: the image is the ADDITIVE row A, and the
	//                  tail reads L per transform as its base pose buffer -- apply_additive_to_base(format, base = L[b], additive = A[b]),
	//                  the roles aclhip_decompress_poses_batch gives an instance's decoded pose and its base_poses row
	//   bounds_types   nothing, or consumer_bounds_launch (object space): a box per instance next to the rows, or in their place
	// Nothing is known about a caller's poses: rtm::qvv_mul's matrix route is always compiled in (kMirrored, the rule the fused kernels
	// apply when the base is a caller's buffer), and short_exact is 0 -- the walk normalizes with the compiler's correctly rounded sqrt and
	// division, because the short forms give the same bits only for rotations of a squared length in their proven range [1/4, 4].
	// In place (poses == local_poses, equal strides): a wave reads its own instance's rows and no other, and every row of the workgroup is
	// complete in LDS -- behind the tail's barriers -- before the first quad of any of them is stored.
	template<bool kObjectSpace, uint32_t kBase, class... bounds_types>
	__global__ __launch_bounds__(k_consumer_max_instances * k_wave_size) void transform_poses_kernel(pose_buffer_launch launch, bounds_types... bounds_launch)
	{
		static_assert(kBase == k_consumer_base_none || kBase == k_consumer_base_buffer, "the additive pose is a caller's buffer, never a clip");
		static_assert(kObjectSpace || kBase == k_consumer_base_buffer, "local space without an additive buffer: nothing to do");
		constexpr bool with_bounds = sizeof...(bounds_types) != 0;
		const pose_rows_shape shape = launch.shape;
		const uint32_t log2_instances_per_block = shape.log2_instances_per_block();
		__shared__ consumer_walk_slots walk;		// (what the host subtracts from the LDS it may ask for: host_consumers.inl)
		ACLHIP_PHASE_STAMP(0);

		consumer_wave wave = consumer_wave_of(log2_instances_per_block, shape.lds_bytes_per_instance, shape.lds_quads_per_image);
		const uint32_t lane = wave.lane, instance = wave.instance;

		// (wave.num_tracks stays 0 for a wave without work: past the batch, refused instance)
		if (instance < shape.num_instances)
		{
			// open_instance's refusal, and more bones than a row of any buffer in use holds
			const opened_instance opened = open_instance<kObjectSpace>(launch.head, shape, instance);
			const uint32_t num_bones = opened.num_bones;
			const uint64_t row_bytes = uint64_t(num_bones) * 48u;
			const bool refused = opened.refused || row_bytes > launch.local_pose_stride_bytes || (launch.poses != nullptr && row_bytes > launch.pose_stride_bytes)
				|| (kBase == k_consumer_base_buffer && row_bytes > launch.additive_pose_stride_bytes);
			if (refused)
				count_refused(shape.rejected_count, lane);
			else if (num_bones != 0)
			{
				wave.num_tracks = num_bones;
				// the walk schedule first: its words travel global -> LDS while the row does
				if (kObjectSpace)
					request_walk_schedule(opened.skeleton.hierarchy, log2_instances_per_block, shape.schedule_words(), wave.shared_schedule, wave.slot, lane, walk);
				// (the tail's first barrier waits for the row)
				fill_image_from_row(wave.image, kBase == k_consumer_base_buffer ? launch.additive_poses + uint64_t(instance) * launch.additive_pose_stride_bytes
					: launch.local_poses + uint64_t(instance) * launch.local_pose_stride_bytes, num_bones * 3u, lane);
			}
			else if constexpr (with_bounds)
				wave.empty_pose = true;		// (a served instance whose pose has no transform)
		}

		// the image of every instance is complete
		wave.short_exact = 0;
		const consumer_bounds_launch bounds = bounds_launch_of(bounds_launch...);
		finish_consumer_poses<kObjectSpace, kBase, false, true, false, with_bounds>(
			consumer_tail_args{ launch.poses, launch.pose_stride_bytes, shape.lds_bytes_per_instance, log2_instances_per_block, shape.rejected_count, launch.local_poses, launch.local_pose_stride_bytes,
				launch.additive_format, bounds.bounds, bounds.bone_flags },
			wave, walk);
	}

	// ---- a blend of K caller pose buffers (aclhip_blend_poses_batch; include/aclhip.h states the definition) -----------------------------
	// the kernel's argument: the K input buffers, the weights and masks of the blend, the output, the tables and the launch's shape
	struct pose_blend_launch
	{
		pose_rows_head head;
		const device_blend_mask* masks;			// the context's mask table (null: no mask was ever registered)
		uint32_t num_masks;						// its capacity
		uint32_t layered;						// ACLHIP_BLEND_LAYERED
		const uint32_t* instance_masks;			// [num_instances * K] or null: every handle 0
		const float* weights;					// [num_instances * K]
		const uint8_t* buffers[ACLHIP_MAX_BLEND_CLIPS];		// row i of buffer k at buffers[k] + i * buffer_stride_bytes[k]
		uint64_t buffer_stride_bytes[ACLHIP_MAX_BLEND_CLIPS];
		uint8_t* poses;							// null: the boxes alone (bounds instantiations)
		uint64_t pose_stride_bytes;
		pose_rows_shape shape;
	};

	// transform_poses_kernel's shape -- one wave64 per instance, images as consumer_wave_of lays them out, open_instance in front of any load
	// of a row -- with the image filled by the masked blend of K rows in the place of one row's DMA:
	//   kNumBuffers    K, a template constant: the K loads of a quad are K independent global_load_dwordx4 in one basic block, requested
	//                  together and waited for once (the launch is bound by its HBM reads), and the accumulation is a straight line over
	//                  registers. The mode and "no masks" are wave uniform data instead: layer_weight's null mask pointer and a weight of
	//                  1 - 0 for a layer that is not above give the definition's bits (slot_weight, kernels_skeleton.inl), at the price of
	//                  a few scalar selects per pass -- 9 instantiations, not 36.
	// Per quad of the row (lanes <-> consecutive quads): e_k = layer_weight's w or w * mask[slot] for every buffer, the weight of buffer k is
	// e_k * r with r the product of (1 - e_j) over the layers above, top layer first, in layered mode and 1 in weighted mode -- what
	// slot_weight computes, with every mask value read once instead of once per layer below it --; buffer 0 is scaled as
	// blend_scale_image scales, buffers 1 .. K - 1 go through blend_accumulate in order, and the sum is written into the LDS image once.
	// blend_normalize_rotations and finish_consumer_poses follow unchanged; short_exact is 0 and the matrix route is compiled in, as for
	// every pose of a caller's.
	// In place (poses == buffers[k], equal strides): a wave reads its own instance's rows and no other, and every row of the workgroup is
	// complete in LDS -- behind the tail's barriers -- before the first quad of any of them is stored.
	template<uint32_t kNumBuffers, bool kObjectSpace, class... bounds_types>
	__global__ __launch_bounds__(k_consumer_max_instances * k_wave_size) void blend_poses_kernel(pose_blend_launch launch, bounds_types... bounds_launch)
	{
		static_assert(kNumBuffers >= 2 && kNumBuffers <= ACLHIP_MAX_BLEND_CLIPS, "a blend of 2 .. ACLHIP_MAX_BLEND_CLIPS buffers");
		constexpr bool with_bounds = sizeof...(bounds_types) != 0;
		const pose_rows_shape shape = launch.shape;
		const uint32_t log2_instances_per_block = shape.log2_instances_per_block();
		__shared__ consumer_walk_slots walk;		// (what the host subtracts from the LDS it may ask for: host_consumers.inl)
		ACLHIP_PHASE_STAMP(0);

		consumer_wave wave = consumer_wave_of(log2_instances_per_block, shape.lds_bytes_per_instance, shape.lds_quads_per_image);
		const uint32_t lane = wave.lane, instance = wave.instance;

		// (wave.num_tracks stays 0 for a wave without work: past the batch, refused instance)
		if (instance < shape.num_instances)
		{
			// open_instance's refusal, over every stride in use ...
			const opened_instance opened = open_instance<kObjectSpace>(launch.head, shape, instance);
			const uint32_t num_bones = opened.num_bones;
			const uint64_t row_bytes = uint64_t(num_bones) * 48u;
			bool refused = opened.refused || (launch.poses != nullptr && row_bytes > launch.pose_stride_bytes);
			// ... and every mask the instance names: the null handle, or a known mask of this skeleton's slot count. The instance's K
			// weights and K mask images on the scalar unit, next to the check.
			layer_weight layers[kNumBuffers];
			const ACLHIP_CONSTANT float* const weights = as_constant(launch.weights) + size_t(instance) * kNumBuffers;
			#pragma unroll
			for (uint32_t k = 0; k < kNumBuffers; ++k)
			{
				refused = refused || row_bytes > launch.buffer_stride_bytes[k];
				const uint32_t mask_id = launch.instance_masks != nullptr ? as_constant(launch.instance_masks)[size_t(instance) * kNumBuffers + k] : 0u;
				const float* mask_image = nullptr;
				if (mask_id != 0)
				{
					const ACLHIP_CONSTANT device_blend_mask* mask_record = as_constant(launch.masks) + (mask_id < launch.num_masks ? mask_id : 0);
					if (mask_id >= launch.num_masks || mask_record->image == nullptr || mask_record->num_slots != num_bones)
						refused = true;
					else
						mask_image = mask_record->image;
				}
				layers[k] = layer_weight{ as_constant(mask_image), weights[k] };
			}

			if (refused)
				count_refused(shape.rejected_count, lane);
			else if (num_bones != 0)
			{
				wave.num_tracks = num_bones;
				// the walk schedule first: its words travel global -> LDS while the rows do
				if (kObjectSpace)
					request_walk_schedule(opened.skeleton.hierarchy, log2_instances_per_block, shape.schedule_words(), wave.shared_schedule, wave.slot, lane, walk);
				const f32x4* sources[kNumBuffers];
				#pragma unroll
				for (uint32_t k = 0; k < kNumBuffers; ++k)
					sources[k] = reinterpret_cast<const f32x4*>(launch.buffers[k] + uint64_t(instance) * launch.buffer_stride_bytes[k]);
				const bool layered = launch.layered != 0;
				// (a mask of the instance's, when it has one: served instances only name known masks of num_bones slots)
				const ACLHIP_CONSTANT float* some_mask = nullptr;
				#pragma unroll
				for (uint32_t k = 0; k < kNumBuffers; ++k)
					some_mask = layers[k].mask != nullptr ? layers[k].mask : some_mask;
				const uint32_t num_quads = num_bones * 3u;
				for (uint32_t base = 0; base < num_quads; base += k_wave_size)
				{
					const uint32_t quad = base + lane;
					if (quad < num_quads)
					{
						// all K quads requested together, then the mask values (the vector cache: a mask is a few hundred bytes every wave reads)
						// and ONE wait for all of them
						f32x4 values[kNumBuffers];
						#pragma unroll
						for (uint32_t k = 0; k < kNumBuffers; ++k)
							values[k] = sources[k][quad];
						const uint32_t slot = quad / 3u;
						const uint32_t kind = quad - slot * 3u;
						// e_k = layer_weight's w, or w * mask[slot]: with a mask among the K, K loads without a branch between them (a
						// layer without one reads another layer's value and keeps its w: a branch per layer made each load wait for
						// the one before it, and for the rows)
						float opacities[kNumBuffers];
						#pragma unroll
						for (uint32_t k = 0; k < kNumBuffers; ++k)
							opacities[k] = layers[k].weight;
						if (some_mask != nullptr)
						{
							float mask_values[kNumBuffers];
							#pragma unroll
							for (uint32_t k = 0; k < kNumBuffers; ++k)
								mask_values[k] = (layers[k].mask != nullptr ? layers[k].mask : some_mask)[slot];
							// (a select between two values that both exist, not a branch around the product: a value that is used under
							// a branch only has its load moved there, behind a wait for everything in front of it)
							#pragma unroll
							for (uint32_t k = 0; k < kNumBuffers; ++k)
							{
								const bool has_mask = layers[k].mask != nullptr;
								const float weight = layers[k].weight, masked = weight * mask_values[k];
								opacities[k] = has_mask ? masked : weight;
							}
						}
						float slot_weights[kNumBuffers];
						float rest = 1.0f;
						#pragma unroll
						for (uint32_t k = kNumBuffers; k-- != 0;)
						{
							slot_weights[k] = opacities[k] * rest;
							rest = layered ? rest * (1.0f - opacities[k]) : 1.0f;
						}
						// buffer 0 times its weight (blend_scale_image), then the others onto it in order (blend_accumulate)
						const float first_weight = slot_weights[0];
						f32x4 accumulated{ values[0].x * first_weight, values[0].y * first_weight, values[0].z * first_weight, kind == 0 ? values[0].w * first_weight : 0.0f };
						#pragma unroll
						for (uint32_t k = 1; k < kNumBuffers; ++k)
							accumulated = blend_accumulate(kind, accumulated, make_float4(values[k].x, values[k].y, values[k].z, values[k].w), slot_weights[k]);
						wave.image[quad] = accumulated;
					}
				}
				wave_lds_barrier();		// every quad has its sum
				blend_normalize_rotations(wave.image, num_bones, lane);
			}
			else if constexpr (with_bounds)
				wave.empty_pose = true;		// (a served instance whose pose has no transform)
		}

		// the image of every instance is complete
		wave.short_exact = 0;
		const consumer_bounds_launch bounds = bounds_launch_of(bounds_launch...);
		finish_consumer_poses<kObjectSpace, k_consumer_base_none, false, true, false, with_bounds>(
			consumer_tail_args{ launch.poses, launch.pose_stride_bytes, shape.lds_bytes_per_instance, log2_instances_per_block, shape.rejected_count, nullptr, 0,
				ACLHIP_ADDITIVE_NONE, bounds.bounds, bounds.bone_flags },
			wave, walk);
	}

	// ---- the way back: object -> local space and make-additive over caller pose buffers (aclhip_inverse_transform_poses_batch) ------------
	// the kernel's argument: the launch's three buffers between the two shared ends (a shape of 0 schedule words: there is no walk)
	struct pose_inverse_launch
	{
		pose_rows_head head;
		const uint8_t* source_poses;			// row i at source_poses + i * source_pose_stride_bytes
		uint64_t source_pose_stride_bytes;
		const uint8_t* base_poses;				// kBase: row i at base_poses + i * base_pose_stride_bytes
		uint64_t base_pose_stride_bytes;
		uint8_t* poses;
		uint64_t pose_stride_bytes;
		uint32_t additive_format;
		pose_rows_shape shape;
	};

	// lhs first, then rhs, with rtm::qvv_mul's matrix route where a scale of either side is negative; the products that take it are counted
	// (aclhip_get_negative_scale_count), one atomic per wave. Called where every lane that is active has a product.
	__device__ __forceinline__ qvv qvv_mul_counted(const qvv& lhs, const qvv& rhs, unsigned long long* negative_scale_count, uint32_t lane)
	{
		const bool through_matrices = qvv_mul_takes_matrix_path(lhs, rhs);
		const uint64_t mirrored = __ballot(through_matrices);
		if (mirrored != 0 && lane == uint32_t(__builtin_ctzll(mirrored)))
			atomicAdd(negative_scale_count, (unsigned long long)__builtin_popcountll(mirrored));
		qvv result = qvv_mul(lhs, rhs);
		if (mirrored != 0 && through_matrices)
			result = qvv_mul_through_matrices(lhs, rhs);
		return result;
	}

	// convert_to_relative / convert_to_additive0 / convert_to_additive1 (core/additive_utils.h:176-195) in the reference's operation order;
	// nothing is normalized there and nothing is here
	__device__ __forceinline__ qvv convert_to_additive(uint32_t additive_format, const qvv& base, const qvv& transform, unsigned long long* negative_scale_count, uint32_t lane)
	{
		if (additive_format == 1)
			return qvv_mul_counted(transform, qvv_inverse(base), negative_scale_count, lane);
		qvv result;
		result.rotation = quat_mul(transform.rotation, make_float4(-base.rotation.x, -base.rotation.y, -base.rotation.z, base.rotation.w));
		result.translation = make_float4(transform.translation.x - base.translation.x, transform.translation.y - base.translation.y, transform.translation.z - base.translation.z, 0.0f);
		if (additive_format == 2)
			result.scale = make_float4(transform.scale.x / base.scale.x, transform.scale.y / base.scale.y, transform.scale.z / base.scale.z, 0.0f);
		else
			result.scale = make_float4((transform.scale.x * (1.0f / base.scale.x)) - 1.0f, (transform.scale.y * (1.0f / base.scale.y)) - 1.0f, (transform.scale.z * (1.0f / base.scale.z)) - 1.0f, 0.0f);
		return result;
	}

	// transform_poses_kernel's shape -- one wave64 per instance, images as consumer_wave_of lays them out, open_instance in front of any load
	// of a row, fill_image_from_row -- and then no walk: a bone's local transform is
	// qvv_mul(object[bone], qvv_inverse(object[parent])), both operands INPUTS, so every lane has a bone of its own and no wave waits for
	// another (no workgroup barrier anywhere, no walk schedule, a wave without work leaves at once).
	//   kLocalSpace    object -> local space with the parent table of the skeleton's hierarchy image (kernels_bone_object.inl reads the same)
	//   kBase          the make-additive step against the base row in HBM, read per transform as finish_consumer_poses reads its base buffer
	// The image is rewritten in place, lanes <-> bones in passes of 64 from the LAST bone down: parents come before their children
	// (registration enforces it), so a pass over bones [k, k + 64) overwrites only what the passes behind it -- bones < k, parents < k --
	// never read; inside a pass every read is waited for before the first write. Nothing is known about a caller's poses: the matrix route
	// is compiled in and the normalize is the correctly rounded one, as in transform_poses_kernel.
	// In place (poses == source_poses, equal strides): a wave reads its own instance's row and no other, and has it complete in LDS before
	// it stores.
	template<bool kLocalSpace, bool kBase>
	__global__ __launch_bounds__(k_consumer_max_instances * k_wave_size) void inverse_transform_poses_kernel(pose_inverse_launch launch)
	{
		static_assert(kLocalSpace || kBase, "object space without a base buffer: nothing to do");
		const pose_rows_shape shape = launch.shape;
		const consumer_wave wave = consumer_wave_of(shape.log2_instances_per_block(), shape.lds_bytes_per_instance, shape.lds_quads_per_image);
		const uint32_t lane = wave.lane, instance = wave.instance;
		if (instance >= shape.num_instances)
			return;

		// open_instance's refusal, over the strides of this launch
		const opened_instance opened = open_instance<kLocalSpace>(launch.head, shape, instance);
		const device_skeleton& skeleton = opened.skeleton;
		const uint32_t num_bones = opened.num_bones;
		const uint64_t row_bytes = uint64_t(num_bones) * 48u;
		const bool refused = opened.refused || row_bytes > launch.source_pose_stride_bytes || row_bytes > launch.pose_stride_bytes
			|| (kBase && row_bytes > launch.base_pose_stride_bytes);
		if (refused)
		{
			count_refused(shape.rejected_count, lane);
			return;
		}
		if (num_bones == 0)
			return;

		// the parent words of the first pass (the last bones) travel while the row does: parent | ancestors << 16, 0xFFFF for a root
		const uint32_t num_passes = (num_bones + k_wave_size - 1) / k_wave_size;
		[[maybe_unused]] const ACLHIP_CONSTANT uint32_t* parents = nullptr;
		[[maybe_unused]] uint32_t parent_word = 0xFFFFu;
		if constexpr (kLocalSpace)
		{
			parents = as_constant(skeleton.hierarchy) + as_constant(skeleton.hierarchy)[3];
			const uint32_t bone = (num_passes - 1u) * k_wave_size + lane;
			if (bone < num_bones)
				parent_word = parents[bone];
		}

		f32x4* const image = wave.image;
		const uint32_t num_quads = num_bones * 3u;
		fill_image_from_row(image, launch.source_poses + uint64_t(instance) * launch.source_pose_stride_bytes, num_quads, lane);
		wave_lds_barrier();		// the row is complete (vmcnt)

		unsigned long long* const negative_scale_count = shape.rejected_count + 1;
		[[maybe_unused]] const f32x4* base_row = kBase ? reinterpret_cast<const f32x4*>(launch.base_poses + uint64_t(instance) * launch.base_pose_stride_bytes) : nullptr;
		for (uint32_t pass = num_passes; pass-- != 0;)
		{
			const uint32_t bone = pass * k_wave_size + lane;
			const uint32_t parent = parent_word & 0xFFFFu;
			// the next pass's parent words are asked for in front of this pass's arithmetic
			if constexpr (kLocalSpace)
			{
				parent_word = 0xFFFFu;
				if (pass != 0)
					parent_word = parents[bone - k_wave_size];
			}
			const bool has_parent = kLocalSpace && bone < num_bones && parent != 0xFFFFu;
			// a root of a launch without a base keeps the bytes of the input, pads included: it is not written
			const bool written = kBase ? bone < num_bones : has_parent;
			qvv result;
			if (written)
			{
				result = load_qvv(image, bone);
				if constexpr (kLocalSpace)
				{
					if (has_parent)
					{
						result = qvv_mul_counted(result, qvv_inverse(load_qvv(image, parent)), negative_scale_count, lane);
						result.rotation = quat_normalize(result.rotation);
					}
				}
				if constexpr (kBase)
					result = convert_to_additive(launch.additive_format, load_qvv(base_row, bone), result, negative_scale_count, lane);
			}
			wave_lds_barrier();		// every read of the pass is behind the wave
			if (written)
				store_qvv(image, bone, result);
			wave_lds_barrier();		// and every write in front of the next pass's reads, and of the store below
		}

		f32x4* pose = reinterpret_cast<f32x4*>(launch.poses + uint64_t(instance) * launch.pose_stride_bytes);
		for (uint32_t quad = lane; quad < num_quads; quad += k_wave_size)
			store_streaming(&pose[quad], image[quad]);
	}

	// ---- 3x4 matrices of caller pose buffers (aclhip_pose_matrices_batch; include/aclhip.h states the definition) -------------------------
	// rtm::matrix3x4f as the reference's matrix error metric uses it (compression/transform_error_metrics.h:389-462): row vectors, point *
	// matrix. Twelve floats: lane 3 of an axis is not part of the value and is not kept. In an LDS image a bone's matrix takes the three
	// quads its QVV record took: x_axis.xyz y_axis.x | y_axis.yz z_axis.xy | z_axis.z w_axis.xyz.
	struct matrix3x4 { float4 x_axis, y_axis, z_axis, w_axis; };

	__device__ __forceinline__ matrix3x4 load_matrix(const f32x4* image, uint32_t transform_index)
	{
		const f32x4 a = image[transform_index * 3u + 0], b = image[transform_index * 3u + 1], c = image[transform_index * 3u + 2];
		return matrix3x4{ make_float4(a.x, a.y, a.z, 0.0f), make_float4(a.w, b.x, b.y, 0.0f), make_float4(b.z, b.w, c.x, 0.0f), make_float4(c.y, c.z, c.w, 0.0f) };
	}

	__device__ __forceinline__ void store_matrix(f32x4* image, uint32_t transform_index, const matrix3x4& value)
	{
		image[transform_index * 3u + 0] = f32x4{ value.x_axis.x, value.x_axis.y, value.x_axis.z, value.y_axis.x };
		image[transform_index * 3u + 1] = f32x4{ value.y_axis.y, value.y_axis.z, value.z_axis.x, value.z_axis.y };
		image[transform_index * 3u + 2] = f32x4{ value.z_axis.z, value.w_axis.x, value.w_axis.y, value.w_axis.z };
	}

	// rtm::matrix_from_qvv: nothing is assumed about the rotation's length or the scale's sign
	__device__ __forceinline__ matrix3x4 matrix_from_qvv(const qvv& transform)
	{
		const float x = transform.rotation.x, y = transform.rotation.y, z = transform.rotation.z, w = transform.rotation.w;
		const float x2 = x + x, y2 = y + y, z2 = z + z;
		const float xx = x * x2, xy = x * y2, xz = x * z2, yy = y * y2, yz = y * z2, zz = z * z2, wx = w * x2, wy = w * y2, wz = w * z2;
		const float sx = transform.scale.x, sy = transform.scale.y, sz = transform.scale.z;
		matrix3x4 result;
		result.x_axis = make_float4((1.0f - (yy + zz)) * sx, (xy + wz) * sx, (xz - wy) * sx, 0.0f);
		result.y_axis = make_float4((xy - wz) * sy, (1.0f - (xx + zz)) * sy, (yz + wx) * sy, 0.0f);
		result.z_axis = make_float4((xz + wy) * sz, (yz - wx) * sz, (1.0f - (xx + yy)) * sz, 0.0f);
		result.w_axis = make_float4(transform.translation.x, transform.translation.y, transform.translation.z, 0.0f);
		return result;
	}

	// rtm::matrix_mul_vector3: ((x_axis * v.x) + y_axis * v.y) + z_axis * v.z, all three products made
	__device__ __forceinline__ float4 matrix_mul_vector3(float x, float y, float z, const matrix3x4& matrix)
	{
		return make_float4(((matrix.x_axis.x * x) + (matrix.y_axis.x * y)) + (matrix.z_axis.x * z), ((matrix.x_axis.y * x) + (matrix.y_axis.y * y)) + (matrix.z_axis.y * z),
			((matrix.x_axis.z * x) + (matrix.y_axis.z * y)) + (matrix.z_axis.z * z), 0.0f);
	}

	// rtm::matrix_mul_point3: the same, and the translation added last
	__device__ __forceinline__ float4 matrix_mul_point3(float x, float y, float z, const matrix3x4& matrix)
	{
		const float4 rotated = matrix_mul_vector3(x, y, z, matrix);
		return make_float4(rotated.x + matrix.w_axis.x, rotated.y + matrix.w_axis.y, rotated.z + matrix.w_axis.z, 0.0f);
	}

	// rtm::matrix_mul: lhs first, then rhs
	__device__ __forceinline__ matrix3x4 matrix_mul(const matrix3x4& lhs, const matrix3x4& rhs)
	{
		matrix3x4 result;
		result.x_axis = matrix_mul_vector3(lhs.x_axis.x, lhs.x_axis.y, lhs.x_axis.z, rhs);
		result.y_axis = matrix_mul_vector3(lhs.y_axis.x, lhs.y_axis.y, lhs.y_axis.z, rhs);
		result.z_axis = matrix_mul_vector3(lhs.z_axis.x, lhs.z_axis.y, lhs.z_axis.z, rhs);
		result.w_axis = matrix_mul_point3(lhs.w_axis.x, lhs.w_axis.y, lhs.w_axis.z, rhs);
		return result;
	}

	// a wave's image rewritten in place, a bone per lane: every QVV record becomes its matrix in the same three quads (a lane reads and
	// writes its own bone's quads and no other)
	__device__ __forceinline__ void convert_image_to_matrices(f32x4* image, uint32_t num_bones, uint32_t lane)
	{
		for (uint32_t bone = lane; bone < num_bones; bone += k_wave_size)
			store_matrix(image, bone, matrix_from_qvv(load_qvv(image, bone)));
	}

	// walk_hierarchy (kernels_consumers.inl) over images of matrices: the SAME schedules -- lanes <-> (instance slot, transform of the current
	// step), `first` picks the lane's transform inside a step, a transform's parent was scheduled in an earlier step and is final by the
	// time it is read -- with matrix_mul(local child, object parent) as its body: 63 operations, no normalize, no route to decide, nothing
	// to count.
	template<class schedule_word_type>
	__device__ __forceinline__ void walk_hierarchy_matrices(const schedule_word_type* schedule_words, uint32_t slot_steps, uint32_t first, f32x4* slot_image)
	{
		const uint32_t first_pair = 2u + slot_steps;		// (behind the step ends)
		uint32_t step_start = 0;
		for (uint32_t step = 0; __any(int(step < slot_steps)) != 0; ++step)
		{
			if (step < slot_steps)
			{
				const uint32_t step_end = schedule_words[2 + step];
				const uint32_t pair_index = step_start + first;
				if (pair_index < step_end)
				{
					const uint32_t pair = schedule_words[first_pair + pair_index];		// transform | parent << 16
					store_matrix(slot_image, pair & 0xFFFFu, matrix_mul(load_matrix(slot_image, pair & 0xFFFFu), load_matrix(slot_image, pair >> 16)));
				}
				step_start = step_end;
			}
			wave_lds_barrier();
		}
	}

	// The walk of a workgroup's images by the wave that calls it, as finish_consumer_poses arranges it: the lane's slot, its steps and its
	// schedule from the walk's slots, the shared LDS copy of the schedule when every slot that walks follows the same one, otherwise each
	// slot's own in global memory. role_quads: where the image of the caller's role starts inside a slot (the measure's second image).
	// The selection is the third copy of the one in finish_consumer_poses and in measure_pose_error_kernel's QVVF branch, which stay as
	// they are to keep their registers: a change to the schedule-sharing rule visits all three.
	__device__ __forceinline__ void walk_workgroup_matrices(const consumer_walk_slots& walk, const uint32_t* shared_schedule, uint32_t log2_instances_per_block,
		uint32_t lds_bytes_per_instance, uint32_t role_quads, uint32_t lane)
	{
		extern __shared__ __attribute__((aligned(16))) uint8_t dynamic_lds[];
		const uint32_t walk_slot = lane & ((1u << log2_instances_per_block) - 1u);
		const uint32_t first = lane >> log2_instances_per_block;
		f32x4* slot_image = reinterpret_cast<f32x4*>(dynamic_lds + size_t(walk_slot) * lds_bytes_per_instance) + role_quads;
		const uint32_t slot_steps = walk.levels[walk_slot] & 0x7FFFFFFFu;
		const bool slot_schedule_is_shared = (walk.levels[walk_slot] & 0x80000000u) == 0;
		const uint32_t* slot_schedule = walk.schedules[walk_slot];
		// the rest of the workgroup waits for this wave: it goes first on its SIMD
		__builtin_amdgcn_s_setprio(3);
		const uint64_t walkers = __ballot(slot_steps != 0);
		if (walkers != 0)
		{
			const uint32_t leader = uint32_t(__builtin_ctzll(walkers));
			const uint64_t mine = reinterpret_cast<uint64_t>(slot_schedule);
			const uint64_t first_schedule = (uint64_t(__shfl(uint32_t(mine >> 32), int(leader))) << 32) | __shfl(uint32_t(mine), int(leader));
			const bool shared_copy = __all(int(slot_steps == 0 || (mine == first_schedule && slot_schedule_is_shared))) != 0;
			if (shared_copy)
				walk_hierarchy_matrices(shared_schedule, slot_steps, first, slot_image);
			else
				walk_hierarchy_matrices(as_constant(slot_schedule), slot_steps, first, slot_image);
		}
		__builtin_amdgcn_s_setprio(0);
	}

	// the kernel's argument: the launch's two buffers between the two shared ends
	struct pose_matrices_launch
	{
		pose_rows_head head;
		const uint8_t* local_poses;				// row i at local_poses + i * local_pose_stride_bytes: QVV48
		uint64_t local_pose_stride_bytes;
		uint8_t* matrices;						// row i at matrices + i * matrix_stride_bytes: 64 bytes per bone
		uint64_t matrix_stride_bytes;
		pose_rows_shape shape;
	};

	// a finished image of matrices into its output row, lanes <-> consecutive OUTPUT quads (a wave writes contiguous pieces of 1 KiB): the
	// three floats of an axis from the image's twelve per bone, and the lane that is no part of the matrix -- +0 for the three axes, 1 for
	// w_axis
	__device__ __forceinline__ void store_matrix_row(const f32x4* image, uint32_t num_bones, uint8_t* row, uint32_t lane)
	{
		const float* floats = reinterpret_cast<const float*>(image);
		f32x4* out = reinterpret_cast<f32x4*>(row);
		const uint32_t num_quads = num_bones * 4u;
		for (uint32_t quad = lane; quad < num_quads; quad += k_wave_size)
		{
			const uint32_t axis = quad & 3u;
			const float* source = floats + (quad >> 2) * 12u + axis * 3u;
			store_streaming(&out[quad], f32x4{ source[0], source[1], source[2], axis == 3u ? 1.0f : 0.0f });
		}
	}

	// pose_matrices_kernel's rows: its clause of the refusal -- 64 bytes per bone on the output side -- and store_matrix_row
	struct matrix_row_writer
	{
		uint8_t* matrices;
		uint64_t matrix_stride_bytes;
		__device__ __forceinline__ bool refuses(uint32_t, uint32_t num_bones) const { return uint64_t(num_bones) * 64u > matrix_stride_bytes; }
		__device__ __forceinline__ void store(const f32x4* image, uint32_t num_bones, uint32_t instance, uint32_t lane) const
		{
			store_matrix_row(image, num_bones, matrices + uint64_t(instance) * matrix_stride_bytes, lane);
		}
	};

	// The body of pose_matrices_kernel and skinning_matrices_kernel, which differ in their `writer` alone. transform_poses_kernel's front
	// -- one wave64 per instance, up to 8 instances per workgroup, images as consumer_wave_of lays them out, open_instance in front of any
	// load of a row, fill_image_from_row behind the request for the walk schedule -- over the rows at `rows`, and then the matrix
	// arithmetic: every wave rewrites its image as matrices (a bone per lane), with
	//   kObjectSpace   ONE wave of the workgroup (it rotates with the workgroup index) walks all its images with walk_hierarchy_matrices
	//                  and then stores all of them, as finish_consumer_poses does for QVV rows; without it every wave stores its own.
	//   writer         refuses(instance, num_bones): its clauses of the refusal, asked once per instance by the instance's own wave;
	//                  store(image, num_bones, instance, lane): a finished image into its output row, num_bones 0 for an image without work
	// Nothing is normalized, routed or counted. The output never overlaps the input (the host refuses it: records differ in size).
	// Every wave of the workgroup reaches the __syncthreads: a wave without work (past the batch, refused, no bones) has num_bones 0.
	template<bool kObjectSpace, class row_writer_type>
	__device__ __forceinline__ void matrices_of_pose_rows(pose_rows_head head, pose_rows_shape shape, const uint8_t* rows, uint64_t row_stride_bytes, row_writer_type writer)
	{
		extern __shared__ __attribute__((aligned(16))) uint8_t dynamic_lds[];
		const uint32_t log2_instances_per_block = shape.log2_instances_per_block();
		__shared__ consumer_walk_slots walk;		// (what the host subtracts from the LDS it may ask for: host_consumers.inl)

		const consumer_wave wave = consumer_wave_of(log2_instances_per_block, shape.lds_bytes_per_instance, shape.lds_quads_per_image);
		const uint32_t lane = wave.lane, instance = wave.instance, slot = wave.slot;
		uint32_t num_bones = 0;

		if (instance < shape.num_instances)
		{
			// open_instance's refusal, more bones than a pose row holds, and what the writer refuses
			const opened_instance opened = open_instance<kObjectSpace>(head, shape, instance);
			const bool writer_refuses = writer.refuses(instance, opened.num_bones);
			if (opened.refused || uint64_t(opened.num_bones) * 48u > row_stride_bytes || writer_refuses)
				count_refused(shape.rejected_count, lane);
			else if (opened.num_bones != 0)
			{
				num_bones = opened.num_bones;
				// the walk schedule first: its words travel global -> LDS while the row does
				if (kObjectSpace)
					request_walk_schedule(opened.skeleton.hierarchy, log2_instances_per_block, shape.schedule_words(), wave.shared_schedule, slot, lane, walk);
				fill_image_from_row(wave.image, rows + uint64_t(instance) * row_stride_bytes, num_bones * 3u, lane);
			}
		}
		wave_lds_barrier();		// the wave's row is complete (vmcnt)
		convert_image_to_matrices(wave.image, num_bones, lane);

		if constexpr (kObjectSpace)
		{
			if (lane == 0)
			{
				close_idle_walk_slot(walk, slot, num_bones);
				walk.tracks[slot] = num_bones;
			}
			__syncthreads();
			// ONE wave walks and then stores the workgroup's rows; the others are done (finish_consumer_poses says why, and why it rotates)
			if (wave.wave_in_block != (blockIdx.x & ((blockDim.x / k_wave_size) - 1u)))
				return;
			walk_workgroup_matrices(walk, wave.shared_schedule, log2_instances_per_block, shape.lds_bytes_per_instance, 0, lane);
			wave_lds_barrier();
			const uint32_t instances_per_block = 1u << log2_instances_per_block;
			for (uint32_t store_slot = 0; store_slot < instances_per_block; ++store_slot)
				writer.store(reinterpret_cast<const f32x4*>(dynamic_lds + size_t(store_slot) * shape.lds_bytes_per_instance), walk.tracks[store_slot],
					(blockIdx.x << log2_instances_per_block) + store_slot, lane);
		}
		else
		{
			wave_lds_barrier();		// every bone has its matrix
			writer.store(wave.image, num_bones, instance, lane);
		}
	}

	template<bool kObjectSpace>
	__global__ __launch_bounds__(k_consumer_max_instances * k_wave_size) void pose_matrices_kernel(pose_matrices_launch launch)
	{
		matrices_of_pose_rows<kObjectSpace>(launch.head, launch.shape, launch.local_poses, launch.local_pose_stride_bytes, matrix_row_writer{ launch.matrices, launch.matrix_stride_bytes });
	}

	// ---- skinning matrix palettes of caller pose buffers (aclhip_skinning_matrices_batch; include/aclhip.h states the definition) ---------
	// A skin's record in the context's skin table (which never moves, like the skeleton table) and its device image: the joint list,
	// num_joints bone indices, and the inverse bind matrices, twelve floats per joint in the three quads load_matrix reads (lane 3 of the
	// caller's axes is dropped at registration). A cleared record (inverse_bind == null) is an unknown or retired skin; record 0 is never
	// handed out. Both arrays are always there: an identity list and identity matrices are stored like any others.
	struct device_skin
	{
		const uint32_t* joint_bones;		// [num_joints] the skeleton bone a joint follows, each < num_bones
		const f32x4* inverse_bind;			// [3 * num_joints] x_axis.xyz y_axis.x | y_axis.yz z_axis.xy | z_axis.z w_axis.xyz per joint
		uint32_t num_joints;
		uint32_t num_bones;					// of the skeleton the skin was made for
		uint32_t flags;						// k_skin_*: what registration found, for whoever reads the table; NO kernel branches on them (see below)
		uint32_t reserved;
	};
	static_assert(sizeof(device_skin) == 32, "load_entry: two dwordx4 loads");
	constexpr uint32_t k_skin_identity_joint_list = 1u << 0;	// joint_bones[j] == j and num_joints == num_bones
	constexpr uint32_t k_skin_has_inverse_bind = 1u << 1;		// registered with matrices (not NULL: identity)
	// The flags are informational. The store always reads the joint list and always makes the product, with an identity list and identity
	// matrices too: 0 * NaN is what carries a NaN or an infinity of bone k[j] into every float of joint j, as the header defines. A
	// shortcut that copies O[k[j]] when a flag is set would write different bits for such rows.

	// a skin's record with every field in scalar registers of its own (load_skeleton_fields, kernels_skeleton.inl, says why)
	__device__ __forceinline__ device_skin load_skin_fields(const device_skin* table, uint32_t index)
	{
		device_skin skin = load_entry(table, index);
		asm volatile("" : "+s"(skin.joint_bones), "+s"(skin.inverse_bind), "+s"(skin.num_joints), "+s"(skin.num_bones));
		return skin;
	}

	constexpr uint32_t k_palette_3x4f_64 = 0, k_palette_3x4f_transposed_48 = 1;		// aclhip_palette_layout

	// the kernel's argument: pose_matrices_launch with the context's skin table and the launch's skins
	struct skinning_matrices_launch
	{
		pose_rows_head head;
		const device_skin* skins;				// the context's skin table
		uint32_t num_skins;						// its capacity
		uint32_t skin;							// the launch's skin, when instance_skins is null
		const uint32_t* instance_skins;			// [num_instances] or null
		const uint8_t* poses;					// row i at poses + i * pose_stride_bytes: QVV48
		uint64_t pose_stride_bytes;
		uint8_t* palettes;						// row i at palettes + i * palette_stride_bytes: 64 or 48 bytes per joint
		uint64_t palette_stride_bytes;
		pose_rows_shape shape;
	};

	// A finished image of object matrices into its palette row: S[j] = matrix_mul(IB[j], O[k[j]]), lanes <-> consecutive OUTPUT quads as in
	// store_matrix_row (a wave writes contiguous pieces of 1 KiB). A lane computes exactly the four floats it stores:
	//   transposed   quad q is row r = q % 3 of joint q / 3 -- component r of the four rows of the product: the lane reads IB[j] whole (three
	//                quads that its two neighbours read as well) and the four floats of column r of O[k[j]] from the image
	//   64 bytes     quad q is axis a = q & 3 of joint q >> 2 -- matrix_mul_vector3 (a < 3) or matrix_mul_point3 (a == 3) of row a of IB[j]
	//                with O[k[j]], read whole from the image; lane 3 is the constant store_matrix_row writes
	// in matrix_mul's operation order. The gather by k[j] is the LDS read; the joint list and IB come through the vector cache (every
	// instance of a skin reads the same few KiB).
	template<uint32_t kLayout>
	__device__ __forceinline__ void store_palette_row(const f32x4* image, const uint32_t* joint_bones, const f32x4* inverse_bind, uint32_t num_joints, uint8_t* row, uint32_t lane)
	{
		const float* floats = reinterpret_cast<const float*>(image);
		f32x4* out = reinterpret_cast<f32x4*>(row);
		if constexpr (kLayout == k_palette_3x4f_transposed_48)
		{
			const uint32_t num_quads = num_joints * 3u;
			for (uint32_t quad = lane; quad < num_quads; quad += k_wave_size)
			{
				const uint32_t joint = quad / 3u;
				const uint32_t component = quad - joint * 3u;
				const matrix3x4 bind = load_matrix(inverse_bind, joint);
				const float* object = floats + joint_bones[joint] * 12u + component;
				const float x = object[0], y = object[3], z = object[6], w = object[9];		// x_axis, y_axis, z_axis, w_axis of O at the component
				store_streaming(&out[quad], f32x4{ ((x * bind.x_axis.x) + (y * bind.x_axis.y)) + (z * bind.x_axis.z), ((x * bind.y_axis.x) + (y * bind.y_axis.y)) + (z * bind.y_axis.z),
					((x * bind.z_axis.x) + (y * bind.z_axis.y)) + (z * bind.z_axis.z), (((x * bind.w_axis.x) + (y * bind.w_axis.y)) + (z * bind.w_axis.z)) + w });
			}
		}
		else
		{
			const uint32_t num_quads = num_joints * 4u;
			for (uint32_t quad = lane; quad < num_quads; quad += k_wave_size)
			{
				const uint32_t joint = quad >> 2, axis = quad & 3u;
				const float* bind_row = reinterpret_cast<const float*>(inverse_bind) + joint * 12u + axis * 3u;
				const matrix3x4 object = load_matrix(image, joint_bones[joint]);
				const float4 rotated = matrix_mul_vector3(bind_row[0], bind_row[1], bind_row[2], object);
				// (the w row alone takes the translation: adding a zero to the others would turn a -0 into +0)
				const bool is_point = axis == 3u;
				store_streaming(&out[quad], f32x4{ is_point ? rotated.x + object.w_axis.x : rotated.x, is_point ? rotated.y + object.w_axis.y : rotated.y,
					is_point ? rotated.z + object.w_axis.z : rotated.z, is_point ? 1.0f : 0.0f });
			}
		}
	}

	// skinning_matrices_kernel's rows, and everything about the skin: the skin's record next to the skeleton's on the scalar unit, its
	// clauses of the refusal -- a skin that is unknown, retired (record 0 is never handed out, a cleared record has no inverse_bind) or made
	// for another bone count, more joints than a palette row holds; every joint's bone of what is served (< skin.num_bones at
	// registration) lies inside the image -- and store_palette_row.
	//   kObjectSpace   the walking wave stores every image of the workgroup: it reads the skin of each slot that has work again on the
	//                  scalar unit (a retirement clears a record behind the launches enqueued before it, never inside one); without it a
	//                  wave stores its own image with the record `refuses` read
	template<uint32_t kLayout, bool kObjectSpace>
	struct palette_row_writer
	{
		const device_skin* skins;
		uint32_t num_skins, skin;
		const uint32_t* instance_skins;
		uint8_t* palettes;
		uint64_t palette_stride_bytes;
		device_skin own_skin = {};		// of the wave's own instance: from refuses to the local space store
		static constexpr uint32_t record_bytes = kLayout == k_palette_3x4f_transposed_48 ? 48u : 64u;

		__device__ __forceinline__ uint32_t skin_of(uint32_t instance) const { return instance_skins != nullptr ? as_constant(instance_skins)[instance] : skin; }
		__device__ __forceinline__ bool refuses(uint32_t instance, uint32_t num_bones)
		{
			const uint32_t skin_id = skin_of(instance);
			own_skin = load_skin_fields(skins, skin_id < num_skins ? skin_id : 0);
			return skin_id >= num_skins || own_skin.inverse_bind == nullptr || own_skin.num_bones != num_bones || uint64_t(own_skin.num_joints) * record_bytes > palette_stride_bytes;
		}
		__device__ __forceinline__ void store(const f32x4* image, uint32_t num_bones, uint32_t instance, uint32_t lane) const
		{
			uint8_t* row = palettes + uint64_t(instance) * palette_stride_bytes;
			if constexpr (kObjectSpace)
			{
				// (wave uniform: every lane reads the same word)
				if (__builtin_amdgcn_readfirstlane(num_bones) == 0)
					return;
				// the slot was served: its handle is a live skin's, checked by the slot's own wave
				const device_skin served = load_skin_fields(skins, skin_of(instance));
				store_palette_row<kLayout>(image, served.joint_bones, served.inverse_bind, served.num_joints, row, lane);
			}
			else
				store_palette_row<kLayout>(image, own_skin.joint_bones, own_skin.inverse_bind, num_bones != 0 ? own_skin.num_joints : 0u, row, lane);
		}
	};

	// pose_matrices_kernel with a palette for its store: matrices_of_pose_rows with store_palette_row in the place of store_matrix_row.
	// The object matrices never leave LDS.
	template<bool kObjectSpace, uint32_t kLayout>
	__global__ __launch_bounds__(k_consumer_max_instances * k_wave_size) void skinning_matrices_kernel(skinning_matrices_launch launch)
	{
		matrices_of_pose_rows<kObjectSpace>(launch.head, launch.shape, launch.poses, launch.pose_stride_bytes,
			palette_row_writer<kLayout, kObjectSpace>{ launch.skins, launch.num_skins, launch.skin, launch.instance_skins, launch.palettes, launch.palette_stride_bytes });
	}

	// ---- how far two pose buffers are apart (aclhip_measure_pose_error_batch; include/aclhip.h states the definition) --------------------
	struct pose_error_record { float error; uint32_t bone; };		// aclhip_pose_error
	constexpr uint32_t k_no_bone = 0xFFFFFFFFu;						// ACLHIP_NO_BONE

	// the kernel's argument: the launch's buffers, its shells and its outputs between the two shared ends (two images per instance)
	struct pose_error_launch
	{
		pose_rows_head head;
		const uint8_t* raw_poses;				// row i at raw_poses + i * raw_pose_stride_bytes
		uint64_t raw_pose_stride_bytes;
		const uint8_t* lossy_poses;				// row i at lossy_poses + i * lossy_pose_stride_bytes
		uint64_t lossy_pose_stride_bytes;
		const uint8_t* base_poses;				// kBase: row i at base_poses + i * base_pose_stride_bytes
		uint64_t base_pose_stride_bytes;
		const float* shell_distances;			// [num_shell_distances] or null: shell_distance for every bone
		uint32_t num_shell_distances;
		float shell_distance;
		uint8_t* bone_errors;					// null, or the error of bone b of instance i at bone_errors + i * bone_error_stride_bytes + 4 * b
		uint64_t bone_error_stride_bytes;
		pose_error_record* errors;				// [num_instances]
		uint32_t additive_format;
		pose_rows_shape shape;
	};

	// rtm::qvv_mul_point3: quat_mul_vector3(scale * point, rotation) + translation, all three components of the product multiplied
	__device__ __forceinline__ float4 qvv_mul_point3(float x, float y, float z, const qvv& transform)
	{
		const float4 scaled = make_float4(transform.scale.x * x, transform.scale.y * y, transform.scale.z * z, 0.0f);
		const float4 rotated = quat_mul_vector3(scaled, transform.rotation);
		return make_float4(rotated.x + transform.translation.x, rotated.y + transform.translation.y, rotated.z + transform.translation.z, 0.0f);
	}

	// how far the point (x, y, z) of a bone moved between the raw and the lossy transform
	__device__ __forceinline__ float shell_point_error(float x, float y, float z, const qvv& raw, const qvv& lossy)
	{
		const float4 raw_point = qvv_mul_point3(x, y, z, raw), lossy_point = qvv_mul_point3(x, y, z, lossy);
		const float dx = lossy_point.x - raw_point.x, dy = lossy_point.y - raw_point.y, dz = lossy_point.z - raw_point.z;
		return sqrtf(((dx * dx) + (dy * dy)) + (dz * dz));
	}

	// qvvf_transform_error_metric::calculate_error (compression/transform_error_metrics.h:335-358): the three points at the shell distance
	__device__ __forceinline__ float shell_error(float distance, const qvv& raw, const qvv& lossy)
	{
		const float error_x = shell_point_error(distance, 0.0f, 0.0f, raw, lossy);
		const float error_y = shell_point_error(0.0f, distance, 0.0f, raw, lossy);
		const float error_z = shell_point_error(0.0f, 0.0f, distance, raw, lossy);
		const float error_xy = error_x > error_y ? error_x : error_y;
		return error_xy > error_z ? error_xy : error_z;
	}

	// qvvf_matrix3x4f_transform_error_metric::calculate_error (compression/transform_error_metrics.h:438-461): the same three points through
	// rtm::matrix_mul_point3, all three products of every point made, the zero ones too
	__device__ __forceinline__ float matrix_shell_point_error(float x, float y, float z, const matrix3x4& raw, const matrix3x4& lossy)
	{
		const float4 raw_point = matrix_mul_point3(x, y, z, raw), lossy_point = matrix_mul_point3(x, y, z, lossy);
		const float dx = lossy_point.x - raw_point.x, dy = lossy_point.y - raw_point.y, dz = lossy_point.z - raw_point.z;
		return sqrtf(((dx * dx) + (dy * dy)) + (dz * dz));
	}

	__device__ __forceinline__ float matrix_shell_error(float distance, const matrix3x4& raw, const matrix3x4& lossy)
	{
		const float error_x = matrix_shell_point_error(distance, 0.0f, 0.0f, raw, lossy);
		const float error_y = matrix_shell_point_error(0.0f, distance, 0.0f, raw, lossy);
		const float error_z = matrix_shell_point_error(0.0f, 0.0f, distance, raw, lossy);
		const float error_xy = error_x > error_y ? error_x : error_y;
		return error_xy > error_z ? error_xy : error_z;
	}

	// The wave's greatest error and, among equal ones, the lowest key (a bone, an instance), left in every lane: a butterfly over a total
	// order -- no error here is a NaN (a lane's record starts at -1 and only takes what compares greater) --, so the result is the same
	// whatever the order of the steps. `payload` travels with the winner.
	__device__ __forceinline__ void wave_reduce_worst(float& error, uint32_t& key, uint32_t& payload)
	{
		#pragma unroll
		for (int offset = int(k_wave_size) / 2; offset != 0; offset >>= 1)
		{
			const float other_error = __shfl_xor(error, offset);
			const uint32_t other_key = uint32_t(__shfl_xor(int(key), offset)), other_payload = uint32_t(__shfl_xor(int(payload), offset));
			const bool take = other_error > error || (other_error == error && other_key < key);
			error = take ? other_error : error;
			key = take ? other_key : key;
			payload = take ? other_payload : payload;
		}
	}

	// transform_poses_kernel's front twice over: TWO waves per instance as consumer_wave_of lays them out -- role 0 holds the raw row in the
	// slot's image, role 1 the lossy row in its base image --, open_instance in front of any load of a row, each row into its image by
	// fill_image_from_row. Then what finish_consumer_poses does to one image is done to both, without a store:
	//   kBase          apply_additive_to_base against the base row in HBM, each wave over its own image (the counter moves as for two launches)
	//   kObjectSpace   walk_hierarchy as it is, by the two waves of ONE slot (it rotates with the workgroup index): role 0 walks every raw
	//                  image of the workgroup, role 1 every lossy one, lanes <-> (slot, transform of the step) over the schedule made for
	//                  this many slots. short_exact is 0 and the matrix route is compiled in, as for every pose of a caller's: the images
	//                  hold the bits aclhip_transform_poses_batch would have written.
	// Behind the workgroup's barrier both images of a slot are final and its two waves measure: a bone per lane, the passes of 64 bones dealt
	// out in turn (role 0 the even ones), per lane the scan of track_error.impl.h:358-375 over its bones in ascending order, then the wave's
	// record by wave_reduce_worst; role 1 hands its record over in LDS and role 0 writes the instance's.
	// Every wave of the workgroup reaches every __syncthreads: a wave without work (past the batch, refused, no bones) has num_bones 0.
	//   kMatrices      qvvf_matrix3x4f_transform_error_metric (aclhip_measure_pose_error_metric_batch, ACLHIP_METRIC_QVVF_MATRIX3X4F; never
	//                  with kBase): each wave rewrites its image as matrices behind its DMA, the walk is walk_hierarchy_matrices over the
	//                  same schedules and the measure is matrix_shell_error; nothing is counted. Without it the text is what it was.
	template<bool kObjectSpace, bool kBase, bool kMatrices = false>
	__global__ __launch_bounds__(k_consumer_max_waves * k_wave_size) void measure_pose_error_kernel(pose_error_launch launch)
	{
		static_assert(!(kMatrices && kBase), "the matrix metric takes no additive base");
		extern __shared__ __attribute__((aligned(16))) uint8_t dynamic_lds[];
		const pose_rows_shape shape = launch.shape;
		const uint32_t log2_instances_per_block = shape.log2_instances_per_block();
		__shared__ consumer_walk_slots walk;		// (what the host subtracts from the LDS it may ask for: host_consumers.inl)
		__shared__ pose_error_record second_wave_record[k_consumer_max_instances];

		const consumer_wave wave = consumer_wave_of(log2_instances_per_block, shape.lds_bytes_per_instance, shape.lds_quads_per_image);
		const uint32_t lane = wave.lane, instance = wave.instance, role = wave.role, slot = wave.slot;
		f32x4* const own_image = role == 0 ? wave.image : wave.base_image;
		uint32_t num_bones = 0;

		if (instance < shape.num_instances)
		{
			// open_instance's refusal, over the strides of this launch, and a bone without a place in the error row or in the shell table.
			// Both waves of the instance decide alike.
			const opened_instance opened = open_instance<kObjectSpace>(launch.head, shape, instance);
			const uint32_t skeleton_bones = opened.num_bones;
			const uint64_t row_bytes = uint64_t(skeleton_bones) * 48u;
			const bool refused = opened.refused || row_bytes > launch.raw_pose_stride_bytes || row_bytes > launch.lossy_pose_stride_bytes
				|| (kBase && row_bytes > launch.base_pose_stride_bytes) || (launch.bone_errors != nullptr && uint64_t(skeleton_bones) * 4u > launch.bone_error_stride_bytes)
				|| (launch.shell_distances != nullptr && skeleton_bones > launch.num_shell_distances);
			if (refused || skeleton_bones == 0)
			{
				// "not measured" (refused) and the reference's invalid_track_error (no bones) are the same record
				if (role == 0)
				{
					if (refused)
						count_refused(shape.rejected_count, lane);
					if (lane == 0)
						launch.errors[instance] = pose_error_record{ -1.0f, k_no_bone };
				}
			}
			else
			{
				num_bones = skeleton_bones;
				// the walk schedule first: its words travel global -> LDS while the rows do
				if (kObjectSpace && role == 0)
					request_walk_schedule(opened.skeleton.hierarchy, log2_instances_per_block, shape.schedule_words(), wave.shared_schedule, slot, lane, walk);
				fill_image_from_row(own_image, role == 0 ? launch.raw_poses + uint64_t(instance) * launch.raw_pose_stride_bytes
					: launch.lossy_poses + uint64_t(instance) * launch.lossy_pose_stride_bytes, num_bones * 3u, lane);
			}
		}
		wave_lds_barrier();		// the wave's row is complete (vmcnt)

		[[maybe_unused]] unsigned long long* const negative_scale_count = shape.rejected_count + 1;
		if constexpr (kMatrices)
			convert_image_to_matrices(own_image, num_bones, lane);
		if constexpr (kBase)
		{
			// finish_consumer_poses' combine, the wave over its own image: the image is the additive pose, the base row is read per transform
			const f32x4* base_row = reinterpret_cast<const f32x4*>(launch.base_poses + uint64_t(instance) * launch.base_pose_stride_bytes);
			for (uint32_t bone = lane; bone < num_bones; bone += k_wave_size)
			{
				const qvv additive = load_qvv(own_image, bone);
				const qvv base = load_qvv(base_row, bone);
				store_qvv(own_image, bone, apply_additive_to_base<true>(launch.additive_format, base, additive));
				// additive_clip_format8::relative is a qvv_mul (core/additive_utils.h:128-160)
				const uint64_t mirrored = __ballot(launch.additive_format == 1 && qvv_mul_takes_matrix_path(additive, base));
				if (mirrored != 0 && lane == uint32_t(__builtin_ctzll(mirrored)))
					atomicAdd(negative_scale_count, (unsigned long long)__builtin_popcountll(mirrored));
			}
		}

		if constexpr (kObjectSpace)
		{
			if (lane == 0 && role == 0)
				close_idle_walk_slot(walk, slot, num_bones);
			__syncthreads();
			// the two waves of one slot walk, the others wait at the barrier below
			if (slot == (blockIdx.x & ((1u << log2_instances_per_block) - 1u)))
			{
				if constexpr (kMatrices)
					walk_workgroup_matrices(walk, wave.shared_schedule, log2_instances_per_block, shape.lds_bytes_per_instance, role * shape.lds_quads_per_image, lane);
				else
				{
					const uint32_t walk_slot = lane & ((1u << log2_instances_per_block) - 1u);
					const uint32_t first = lane >> log2_instances_per_block;
					f32x4* slot_image = reinterpret_cast<f32x4*>(dynamic_lds + size_t(walk_slot) * shape.lds_bytes_per_instance) + size_t(role) * shape.lds_quads_per_image;
					const uint32_t slot_steps = walk.levels[walk_slot] & 0x7FFFFFFFu;
					const bool slot_schedule_is_shared = (walk.levels[walk_slot] & 0x80000000u) == 0;
					const uint32_t* slot_schedule = walk.schedules[walk_slot];
					__builtin_amdgcn_s_setprio(3);
					const uint64_t walkers = __ballot(slot_steps != 0);
					if (walkers != 0)
					{
						// all instances that walk follow the same schedule? then the shared LDS copy is theirs; otherwise each reads its own
						// from global memory (finish_consumer_poses). walk_workgroup_matrices above holds the same selection for the matrix
						// walk, kept apart so that this branch compiles to what it was: a change to the rule visits all three
						const uint32_t leader = uint32_t(__builtin_ctzll(walkers));
						const uint64_t mine = reinterpret_cast<uint64_t>(slot_schedule);
						const uint64_t first_schedule = (uint64_t(__shfl(uint32_t(mine >> 32), int(leader))) << 32) | __shfl(uint32_t(mine), int(leader));
						const bool shared_copy = __all(int(slot_steps == 0 || (mine == first_schedule && slot_schedule_is_shared))) != 0;
						if (shared_copy)
							walk_hierarchy<false, true, false, false>(static_cast<const uint32_t*>(wave.shared_schedule), slot_steps, first, slot_image, lane, negative_scale_count);
						else
							walk_hierarchy<false, true, false, false>(as_constant(slot_schedule), slot_steps, first, slot_image, lane, negative_scale_count);
					}
					__builtin_amdgcn_s_setprio(0);
				}
			}
		}
		__syncthreads();		// both images of every slot are final

		// the measure: lanes <-> bones, the passes of 64 dealt out to the instance's two waves in turn
		float worst_error = -1.0f;
		uint32_t worst_bone = k_no_bone;
		{
			const f32x4* raw_image = wave.image;
			const f32x4* lossy_image = wave.base_image;
			const ACLHIP_CONSTANT float* shell_distances = as_constant(launch.shell_distances);
			float* bone_errors = launch.bone_errors != nullptr ? reinterpret_cast<float*>(launch.bone_errors + uint64_t(instance) * launch.bone_error_stride_bytes) : nullptr;
			for (uint32_t bone = role * k_wave_size + lane; bone < num_bones; bone += 2u * k_wave_size)
			{
				const float distance = shell_distances != nullptr ? shell_distances[bone] : launch.shell_distance;
				float error;
				if constexpr (kMatrices)
					error = matrix_shell_error(distance, load_matrix(raw_image, bone), load_matrix(lossy_image, bone));
				else
					error = shell_error(distance, load_qvv(raw_image, bone), load_qvv(lossy_image, bone));
				if (bone_errors != nullptr)
					bone_errors[bone] = error;
				// (a NaN compares false: it never wins)
				if (error > worst_error)
				{
					worst_error = error;
					worst_bone = bone;
				}
			}
		}
		uint32_t unused_payload = 0;
		wave_reduce_worst(worst_error, worst_bone, unused_payload);
		if (role == 1 && lane == 0)
			second_wave_record[slot] = pose_error_record{ worst_error, worst_bone };
		__syncthreads();
		if (role == 0 && lane == 0 && num_bones != 0)
		{
			const pose_error_record other = second_wave_record[slot];
			const bool take = other.error > worst_error || (other.error == worst_error && other.bone < worst_bone);
			launch.errors[instance] = take ? other : pose_error_record{ worst_error, worst_bone };
		}
	}

	// The launch's worst record (aclhip_pose_error_worst): the scan of the instances' records in ascending order -- the greatest error,
	// its bone, the lowest instance that has it; {-1, ACLHIP_NO_BONE, 0xFFFFFFFF, 0} when no record has an error >= 0. ONE workgroup behind
	// the measure on the same stream: a thread scans every 1024th record, the waves reduce, the first wave reduces the waves.
	constexpr uint32_t k_pose_error_worst_threads = 1024;
	__global__ __launch_bounds__(k_pose_error_worst_threads) void pose_error_worst_kernel(const pose_error_record* errors, uint32_t num_instances, u32x4* worst)
	{
		__shared__ float wave_errors[k_pose_error_worst_threads / k_wave_size];
		__shared__ uint32_t wave_instances[k_pose_error_worst_threads / k_wave_size], wave_bones[k_pose_error_worst_threads / k_wave_size];
		const uint32_t lane = threadIdx.x & (k_wave_size - 1), wave_in_block = threadIdx.x / k_wave_size;
		float worst_error = -1.0f;
		uint32_t worst_instance = 0xFFFFFFFFu, worst_bone = k_no_bone;
		for (uint32_t instance = threadIdx.x; instance < num_instances; instance += k_pose_error_worst_threads)
		{
			const pose_error_record record = errors[instance];
			if (record.error > worst_error)
			{
				worst_error = record.error;
				worst_instance = instance;
				worst_bone = record.bone;
			}
		}
		wave_reduce_worst(worst_error, worst_instance, worst_bone);
		if (lane == 0)
		{
			wave_errors[wave_in_block] = worst_error;
			wave_instances[wave_in_block] = worst_instance;
			wave_bones[wave_in_block] = worst_bone;
		}
		__syncthreads();
		if (wave_in_block != 0)
			return;
		const bool has_record = lane < k_pose_error_worst_threads / k_wave_size;
		worst_error = has_record ? wave_errors[lane] : -1.0f;
		worst_instance = has_record ? wave_instances[lane] : 0xFFFFFFFFu;
		worst_bone = has_record ? wave_bones[lane] : k_no_bone;
		wave_reduce_worst(worst_error, worst_instance, worst_bone);
		if (lane == 0)
			*worst = u32x4{ __float_as_uint(worst_error), worst_bone, worst_instance, 0u };
	}
