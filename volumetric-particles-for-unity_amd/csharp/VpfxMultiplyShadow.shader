// VpfxMultiplyShadow.shader -- MetavoxelManager.matMultiplyShadow: multiplies the render target's rgb by the volume-shadow factor image
// (vp_volume_shadow_image, uploaded as an RFloat texture: 1 = fully lit), alpha untouched.  Blit(shadowTex, mainSceneRT, material).
Shader "Hidden/VpfxMultiplyShadow"
{
    Properties { _MainTex ("Shadow factor", 2D) = "white" {} }
    SubShader
    {
        Cull Off ZWrite Off ZTest Always
        Blend DstColor Zero
        ColorMask RGB
        Pass
        {
            CGPROGRAM
            #pragma vertex vert_img
            #pragma fragment frag
            #include "UnityCG.cginc"
            sampler2D _MainTex;
            float4 frag(v2f_img i) : SV_Target
            {
                float s = tex2D(_MainTex, i.uv).r;
                return float4(s, s, s, 1.0);
            }
            ENDCG
        }
    }
}
