package com.android.nQuant;

/* Host class of the MI355X build: same public surface as the reference's PnnQuantizer (constructor from a file name,
 * Bitmap convert(int nMaxColors, boolean dither) throws Exception, boolean hasAlpha()); the quantization itself runs in
 * libnquant_hip.so through the JNI shim jni/nquant_jni.c.  Not compiled in the build image (no JDK there). */

import android.graphics.Bitmap;
import android.graphics.BitmapFactory;

public class PnnQuantizer {
	static { System.loadLibrary("nquant_jni"); }

	public static final int MODE_REFERENCE_SEQUENTIAL = 0, MODE_PARALLEL_TILED = 1, MODE_LOOKUP_ONLY = 2;

	protected int width, height;
	protected int[] pixels = null;
	protected long handle = 0;
	protected int mode = MODE_PARALLEL_TILED;
	protected long seed = System.nanoTime();     // the reference draws from an unseeded java.util.Random
	protected int[] palette = null;

	protected int kind() { return 0; }           // 0 = PnnQuantizer, 1 = PnnLABQuantizer

	private static native long nqCreate(int kind, int device);
	private static native void nqDestroy(long h);
	private static native int[] nqConvert(long h, int[] argb, int w, int hgt, int nMaxColors, boolean dither, long seed, int mode,
	                                      int[] outArgb, short[] outIndex);
	private static native boolean nqHasAlpha(long h);

	public PnnQuantizer(String fname) {
		Bitmap bitmap = BitmapFactory.decodeFile(fname);
		width = bitmap.getWidth();
		height = bitmap.getHeight();
		pixels = new int[width * height];
		bitmap.getPixels(pixels, 0, width, 0, 0, width, height);
	}

	public void setSeed(long seed) { this.seed = seed; }
	public void setMode(int mode) { this.mode = mode; }
	public int[] getPalette() { return palette; }

	public Bitmap convert(int nMaxColors, boolean dither) throws Exception {
		if (handle == 0)
			handle = nqCreate(kind(), 0);
		int[] qPixels = new int[pixels.length];
		palette = nqConvert(handle, pixels, width, height, nMaxColors, dither, seed, mode, qPixels, null);
		return Bitmap.createBitmap(qPixels, width, height, Bitmap.Config.ARGB_8888);
	}

	public boolean hasAlpha() {
		return handle != 0 && nqHasAlpha(handle);
	}

	/** convert() of many quantizer objects in one call (nq_convert_batch): the merge loops of all images run side by side on
	 *  the GPU.  in[i] / out[i] are DIRECT buffers of width*height ints (page-lock them for fully overlapped copies);
	 *  returns the palettes. Results equal quantizers[i].convert(nMaxColors, dither) with the same seed. */
	public static int[][] convertBatch(PnnQuantizer[] quantizers, java.nio.IntBuffer[] in, java.nio.IntBuffer[] out,
			int nMaxColors, boolean dither) {
		long[] handles = new long[quantizers.length], seeds = new long[quantizers.length];
		int[] widths = new int[quantizers.length], heights = new int[quantizers.length];
		for (int i = 0; i < quantizers.length; ++i) {
			PnnQuantizer q = quantizers[i];
			if (q.handle == 0)
				q.handle = nqCreate(q.kind(), 0);
			handles[i] = q.handle; seeds[i] = q.seed; widths[i] = q.width; heights[i] = q.height;
		}
		int[][] palettes = nqConvertBatch(handles, in, widths, heights, nMaxColors, dither, seeds, quantizers[0].mode, out);
		for (int i = 0; i < quantizers.length; ++i)
			quantizers[i].palette = palettes[i];
		return palettes;
	}
	private static native int[][] nqConvertBatch(long[] handles, java.nio.IntBuffer[] in, int[] widths, int[] heights,
			int nMaxColors, boolean dither, long[] seeds, int mode, java.nio.IntBuffer[] out);

	/** One palette for a sequence of frames (nq_convert_frames): an animated GIF's global colour table, a video shot.  The palette
	 *  is what convert() computes for one image holding all frames' pixels one after another; every frame is then dithered as an
	 *  image of its own with that palette and seeds[i].  in[i] / out[i] are DIRECT buffers of widths[i]*heights[i] ints; kind: 0 =
	 *  PnnQuantizer, 1 = PnnLABQuantizer.  Returns the palette. */
	public static int[] convertFrames(int kind, java.nio.IntBuffer[] in, int[] widths, int[] heights, int nMaxColors, boolean dither,
			long[] seeds, java.nio.IntBuffer[] out) {
		long h = nqCreate(kind, 0);
		try {
			return nqConvertFrames(h, in, widths, heights, nMaxColors, dither, seeds, MODE_PARALLEL_TILED, out);
		} finally {
			nqDestroy(h);
		}
	}
	private static native int[] nqConvertFrames(long h, java.nio.IntBuffer[] in, int[] widths, int[] heights, int nMaxColors,
			boolean dither, long[] seeds, int mode, java.nio.IntBuffer[] out);

	/** A GIF89a file of index maps (nq_encode_gif, encoded on the GPU): index[i] is a DIRECT buffer of widths[i]*heights[i] palette
	 *  indices, palette the ARGB entries (at most 256; the first entry with alpha 0 is the transparent index), delaysCs the per-frame
	 *  delays in hundredths of a second (null: 0), loopCount the NETSCAPE2.0 loop count of an animation (0 = for ever, -1 = none). */
	public static byte[] encodeGif(java.nio.ShortBuffer[] index, int[] widths, int[] heights, int[] palette, int[] delaysCs, int loopCount) {
		java.nio.ByteBuffer out = gifBuffer(widths, heights);
		long h = nqCreate(0, 0);
		try {
			return gifBytes(out, nqEncodeGif(h, index, widths, heights, palette, delaysCs, loopCount, out, out.capacity()));
		} finally {
			nqDestroy(h);
		}
	}
	private static native long nqEncodeGif(long h, java.nio.ShortBuffer[] index, int[] widths, int[] heights, int[] palette, int[] delaysCs,
			int loopCount, java.nio.ByteBuffer out, long cap);

	/** encodeGif in delta mode (nq_encode_gif_delta): all frames are width x height; every frame after the first stores only the
	 *  rectangle that differs from the frame before, its unchanged pixels transparent, and keeps the canvas.  With two frames or more
	 *  the palette must not hold an entry with alpha 0. */
	public static byte[] encodeGifDelta(java.nio.ShortBuffer[] index, int width, int height, int[] palette, int[] delaysCs, int loopCount) {
		int[] widths = new int[index.length], heights = new int[index.length];
		java.util.Arrays.fill(widths, width);
		java.util.Arrays.fill(heights, height);
		java.nio.ByteBuffer out = gifBuffer(widths, heights);
		long h = nqCreate(0, 0);
		try {
			return gifBytes(out, nqEncodeGifDelta(h, index, width, height, palette, delaysCs, loopCount, out, out.capacity()));
		} finally {
			nqDestroy(h);
		}
	}
	private static native long nqEncodeGifDelta(long h, java.nio.ShortBuffer[] index, int width, int height, int[] palette, int[] delaysCs,
			int loopCount, java.nio.ByteBuffer out, long cap);

	/** convertFrames (one shared palette, every frame dithered with it) followed by encodeGif of the index maps, in one native call;
	 *  nMaxColors <= 256.  in[i] are DIRECT buffers of widths[i]*heights[i] ARGB ints. */
	public static byte[] convertFramesToGif(int kind, java.nio.IntBuffer[] in, int[] widths, int[] heights, int nMaxColors, boolean dither,
			long[] seeds, int[] delaysCs, int loopCount) {
		return convertFramesToGif(kind, in, widths, heights, nMaxColors, dither, seeds, delaysCs, loopCount, false);
	}
	/** The same with delta = true: encodeGifDelta of the index maps; the frames must have one size.  Regions that do not move drop out
	 *  of the file when the seeds are equal (the tiled dither then repeats their indices from frame to frame). */
	public static byte[] convertFramesToGif(int kind, java.nio.IntBuffer[] in, int[] widths, int[] heights, int nMaxColors, boolean dither,
			long[] seeds, int[] delaysCs, int loopCount, boolean delta) {
		java.nio.ByteBuffer out = gifBuffer(widths, heights);
		long h = nqCreate(kind, 0);
		try {
			return gifBytes(out, nqConvertFramesToGif(h, in, widths, heights, nMaxColors, dither, seeds, MODE_PARALLEL_TILED, delaysCs,
					loopCount, delta, out, out.capacity()));
		} finally {
			nqDestroy(h);
		}
	}
	private static native long nqConvertFramesToGif(long h, java.nio.IntBuffer[] in, int[] widths, int[] heights, int nMaxColors,
			boolean dither, long[] seeds, int mode, int[] delaysCs, int loopCount, boolean delta, java.nio.ByteBuffer out, long cap);

	private static java.nio.ByteBuffer gifBuffer(int[] widths, int[] heights) {
		long cap = nqGifMaxBytes(widths, heights);
		if (cap < 0 || cap > Integer.MAX_VALUE)
			throw new IllegalArgumentException("a GIF of these frames does not fit one byte[]");
		return java.nio.ByteBuffer.allocateDirect((int) cap);
	}
	private static byte[] gifBytes(java.nio.ByteBuffer out, long size) {
		byte[] gif = new byte[(int) size];
		out.get(gif);
		return gif;
	}
	/** nq_gif_max_bytes for K = 256 (an upper bound for every K); -1 for invalid sizes */
	private static native long nqGifMaxBytes(int[] widths, int[] heights);

	/** An indexed PNG file of one index map (nq_encode_png, encoded on the GPU): index is a DIRECT buffer of width*height palette
	 *  indices, palette the ARGB entries (at most 256; alpha values other than 255 go to a tRNS chunk, all 8 bits). */
	public static byte[] encodePng(java.nio.ShortBuffer index, int width, int height, int[] palette) {
		java.nio.ByteBuffer out = pngBuffer(width, height);
		long h = nqCreate(0, 0);
		try {
			return gifBytes(out, nqEncodePng(h, index, width, height, palette, out, out.capacity()));
		} finally {
			nqDestroy(h);
		}
	}
	private static native long nqEncodePng(long h, java.nio.ShortBuffer index, int width, int height, int[] palette, java.nio.ByteBuffer out,
			long cap);

	/** convert(nMaxColors, dither) of the kind's quantizer followed by encodePng of the index map, in one native call; nMaxColors <= 256.
	 *  in is a DIRECT buffer of width*height ARGB ints. */
	public static byte[] convertToPng(int kind, java.nio.IntBuffer in, int width, int height, int nMaxColors, boolean dither, long seed) {
		java.nio.ByteBuffer out = pngBuffer(width, height);
		long h = nqCreate(kind, 0);
		try {
			return gifBytes(out, nqConvertToPng(h, in, width, height, nMaxColors, dither, seed, MODE_PARALLEL_TILED, out, out.capacity()));
		} finally {
			nqDestroy(h);
		}
	}
	private static native long nqConvertToPng(long h, java.nio.IntBuffer in, int width, int height, int nMaxColors, boolean dither, long seed,
			int mode, java.nio.ByteBuffer out, long cap);

	private static java.nio.ByteBuffer pngBuffer(int width, int height) {
		long cap = nqPngMaxBytes(width, height);
		if (cap < 0 || cap > Integer.MAX_VALUE)
			throw new IllegalArgumentException("a PNG of this image does not fit one byte[]");
		return java.nio.ByteBuffer.allocateDirect((int) cap);
	}
	/** nq_png_max_bytes of one image for K = 256 (an upper bound for every K); -1 for an invalid size */
	private static native long nqPngMaxBytes(int width, int height);

	/** An animated PNG (APNG) of index maps of one size over one palette (nq_encode_apng, encoded on the GPU): every frame after the
	 *  first stores only the rectangle that differs from the frame before, and all 8 bits of the palette's alpha are kept, so --
	 *  unlike encodeGifDelta -- the palette may hold transparent and translucent entries.  index[i] are DIRECT buffers of width*height
	 *  palette indices; delaysCs in hundredths of a second (null: 0); loopCount 0 plays for ever. */
	public static byte[] encodeApng(java.nio.ShortBuffer[] index, int width, int height, int[] palette, int[] delaysCs, int loopCount) {
		java.nio.ByteBuffer out = apngBuffer(index.length, width, height);
		long h = nqCreate(0, 0);
		try {
			return gifBytes(out, nqEncodeApng(h, index, width, height, palette, delaysCs, loopCount, out, out.capacity()));
		} finally {
			nqDestroy(h);
		}
	}
	private static native long nqEncodeApng(long h, java.nio.ShortBuffer[] index, int width, int height, int[] palette, int[] delaysCs,
			int loopCount, java.nio.ByteBuffer out, long cap);

	/** convertFrames (one shared palette, every frame dithered with it) followed by encodeApng of the index maps, in one native call on
	 *  one handle; nMaxColors <= 256.  in[i] are DIRECT buffers of width*height ARGB ints.  Regions that do not move drop out of the
	 *  file when the seeds are equal (the tiled dither then repeats their indices from frame to frame). */
	public static byte[] convertFramesToApng(int kind, java.nio.IntBuffer[] in, int width, int height, int nMaxColors, boolean dither,
			long[] seeds, int[] delaysCs, int loopCount) {
		java.nio.ByteBuffer out = apngBuffer(in.length, width, height);
		long h = nqCreate(kind, 0);
		try {
			return gifBytes(out, nqConvertFramesToApng(h, in, width, height, nMaxColors, dither, seeds, MODE_PARALLEL_TILED, delaysCs,
					loopCount, out, out.capacity()));
		} finally {
			nqDestroy(h);
		}
	}
	private static native long nqConvertFramesToApng(long h, java.nio.IntBuffer[] in, int width, int height, int nMaxColors,
			boolean dither, long[] seeds, int mode, int[] delaysCs, int loopCount, java.nio.ByteBuffer out, long cap);

	private static java.nio.ByteBuffer apngBuffer(int n, int width, int height) {
		long cap = nqApngMaxBytes(n, width, height);
		if (cap < 0 || cap > Integer.MAX_VALUE)
			throw new IllegalArgumentException("an APNG of these frames does not fit one byte[]");
		return java.nio.ByteBuffer.allocateDirect((int) cap);
	}
	/** nq_apng_max_bytes (an upper bound for every K and any content); -1 for invalid sizes */
	private static native long nqApngMaxBytes(int n, int width, int height);

	@Override
	protected void finalize() throws Throwable {
		if (handle != 0) { nqDestroy(handle); handle = 0; }
		super.finalize();
	}
}
